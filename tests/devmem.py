"""Device buffers at a chosen distance from the 16-byte grid, with guard bytes on both sides (the seam tests of
test_gpu_seam_alignment.py; the patterns are _Device of test_gpu_layouts.py and _device_view of test_gpu_digest.py).  torch is
imported when a view is made, so that a test without a GPU can import the module."""
import numpy as np

GUARD_BYTE = 0x5A


def fill(shape, dtype):
    """A host array of `shape` whose every BYTE is the guard byte: what an output view holds before a call."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.full(n, GUARD_BYTE, np.uint8).view(dtype).reshape(shape)


def view(x, byte_offset, guard=64):
    """x (a numpy array) in a torch device allocation: -> (the view, guards_intact).

    The view has x's shape and dtype, holds x's bytes and starts `byte_offset` bytes behind a 16-byte boundary; at least
    `guard` bytes of 0x5A lie in front of it and behind it.  guards_intact() reads the allocation back and says whether every
    byte outside the view is still 0x5A."""
    import torch
    x = np.ascontiguousarray(x)
    item, nbytes = x.dtype.itemsize, x.size * x.dtype.itemsize
    if not 0 <= byte_offset < 16 or byte_offset % item:
        raise ValueError("offset %d: not in [0, 16) or not a multiple of the element size %d" % (byte_offset, item))
    hold = torch.full((nbytes + 2 * guard + 32,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    start = guard + (-(hold.data_ptr() + guard)) % 16 + byte_offset           # first byte of the view within `hold`
    hold[start: start + nbytes].copy_(torch.from_numpy(x.reshape(-1).view(np.uint8).copy()))
    torch.cuda.synchronize()
    v = hold[start: start + nbytes].view(torch.from_numpy(np.empty(0, x.dtype)).dtype).view(x.shape)
    assert v.data_ptr() % 16 == byte_offset and v.is_contiguous() and start >= guard and hold.numel() - start - nbytes >= guard

    def guards_intact():
        torch.cuda.synchronize()
        h = hold.cpu().numpy()
        return bool((h[:start] == GUARD_BYTE).all() and (h[start + nbytes:] == GUARD_BYTE).all())

    return v, guards_intact


def host(v):
    """The view's content as a numpy array (after a device synchronisation)."""
    import torch
    torch.cuda.synchronize()
    return v.cpu().numpy()
