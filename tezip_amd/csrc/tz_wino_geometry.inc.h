// k_wino / k_wino2 (tz_wino_kernels.hip.h), a section of the kernel body both share as text: work split, tile geometry and the LDS-DMA lane offsets of a workgroup.
    // columns of a block in the start values / biases, and where column tile t of this kernel sits among them: a three-gate
    // launch that starts from G0 / the bias reads the four-gate rows; the second half of a split starts from what the first
    // half wrote, 48 columns a block
    constexpr bool G3 = (EPI == EPI_LSTM3 && !NOSAME) || EPI == EPI_RAW3;
    constexpr int CBW = G3 ? 64 : 16 * NT;
#define TZW_COLT(t) (G3 ? 16 * ((t) + ((t) > 0)) : 16 * (t))
    using namespace tzw;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mt = wv & 3, ph = wv >> 2;
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    // a workgroup walks over `ipw` column blocks of ITS tile one after the other (items): geometry, zero fill and the first
    // DMA round trip happen once, the stream of stages runs on across the items (the first stages of the next item are
    // issued under the last ones of the current)
    const int ipw = a.ipw, ncbg = a.ncb / ipw;
    const int cb0 = (bid % ncbg) * ipw;
    bid /= ncbg;
    const int ntiles = a.tiles_x * a.tiles_y;
    const int tile = bid % ntiles, n = bid / ntiles;
    const int ty0 = (tile / a.tiles_x) * 16, tx0 = (tile % a.tiles_x) * 16;
    const int g = lane >> 4, r = lane & 15;
#ifdef TZW_STAMPS
    int stamp_id = blockIdx.x * a.ipw;   // one record per item
#endif
    TZW_STAMP(0)
#ifdef TZW_STAMPS
    if (tid == 0 && stamp_id < 4096) {   // where this workgroup runs: (XCC, SE, SH, CU) -- slot 7
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hw), "=s"(xcc));
        for (int q = 0; q < a.ipw && stamp_id + q < 4096; ++q) tzw_stamps[(a.ncb & 3) | (EPI == EPI_LSTM ? 4 : 0)][stamp_id + q][7] = ((unsigned long long)(xcc & 15) << 32) | hw;
    }
#endif
    const unsigned sbase = lds_addr(smem);
    const int S1 = NOSAME ? 0 : a.src[0].C >> 2;          // stages of the same-resolution source
    const int S = S1 + (UPS ? a.src[1].C >> 2 : 0);       // ... and of the upsampled one
    const int SI = a.wino_stride ? a.wino_stride : S;     // stages per column block in the image (a launch may walk a part)

    // ---- DMA geometry, once per workgroup.  Same-resolution plane: piece wv = slots 41 wv ..; slot = row * 18 + column
    // with the columns stored evens first.  Half-resolution plane: piece wv = slots 13 wv .., slot = row * 10 + column.
    unsigned poff, uoff = 0;
    unsigned long long pmask, umask = 0;
    {
        const int slot = wv * PP + lane;
        const int py = slot / WPW, xs = slot - py * WPW;
        const int px = xs < WPW / 2 ? 2 * xs : 2 * (xs - WPW / 2) + 1;
        const int yy = ty0 - 1 + py, xx = tx0 - 1 + px;
        const bool ok = lane < PP && slot < WPW * WPW && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
        poff = ok ? 4u * (unsigned)((yy * a.W + xx) * a.src[0].pstride) : 0u;
        pmask = __ballot(ok);
    }
    if (UPS) {
        const int slot = wv * UP + lane;
        const int Y = slot / WLW, X = slot - Y * WLW;
        const int ly = (ty0 >> 1) - 1 + Y, lx = (tx0 >> 1) - 1 + X;
        const bool ok = lane < UP && slot < WLW * WLW && ly >= 0 && ly < (a.H >> 1) && lx >= 0 && lx < (a.W >> 1);
        uoff = ok ? 4u * (unsigned)((ly * (a.W >> 1) + lx) * a.src[1].pstride) : 0u;
        umask = __ballot(ok);
    }
    const unsigned lane16 = lane * 16;
