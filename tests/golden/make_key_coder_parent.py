"""Writes tests/golden/key_coder_parent.json: the scope counts of the 'huffman' profiling class, the TZD64 digests and the
refusal texts that tests/test_gpu_keycoderg.py pins for the key-frame coders (TZK1 and TZK2), as a library gives them on the
GPU.  It was run with the library of the commit before the two coders were put behind one residual path; run it again only
with a library whose key coders are the intended ones.  It needs a GPU and a built library: this tree's
(python -m tezip_amd.build), or another build of the same C ABI given as the argument.

    python tests/golden/make_key_coder_parent.py [libtezip_hip.so]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]

if __name__ == "__main__":
    import torch  # noqa: F401  (first, as under pytest: the library then shares the HIP runtime torch has loaded)
    import test_gpu_keycoderg as T
    if len(sys.argv) > 1:
        from tezip_amd import _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    with open(T.FIXTURE, "w") as f:
        json.dump(T.record(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", T.FIXTURE)
