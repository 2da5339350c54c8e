// k_wino / k_wino2 (tz_wino_kernels.hip.h), a section of the kernel body both share as text: the output transform of an item.
    // ---- output transform, oracle order, one column tile per round (everything of a round dies with it: the first form
    // computed all row sums ahead and the compiler parked them in AGPRs -- 1100 vector instructions per wave with the matrix
    // pipes idle; this one has ~450).
    //   y[0][b] = ((init + Z[0][b]) + Z[1][b]) + Z[2][b] belongs to the wave with rows 0, 1 and needs Z[2] of its partner;
    //   y[1][b] = ((init + Z[1][b]) - Z[2][b]) - Z[3][b] belongs to the wave with rows 2, 3 and needs Z[1]:
    // exchanged through LDS, two areas of 16 KB in turn, so that one barrier a round is enough (a wave that writes area
    // t & 1 again in round t + 2 has passed the barrier of round t + 1, behind which nobody reads round t's data any more)
    f32x4 Y[2][4];
    {
        // accumulator start of this wave's outputs: row a = ph of the tiles, columns b = 0, 1; register e <-> tile (g, e)
        f32x4 in0[NT], in1[NT];
        {
            const int y = ty0 + 8 * (mt >> 1) + 2 * g + ph + per_item, x0 = tx0 + 8 * (mt & 1);
            // (uniform) away from the border of the plane G0 is one value per column (ConvArgs::init_u): NT loads and a
            // splat, the bias branch below, instead of 8 NT scattered ones
            const bool uni_init = tile_uniform(a.init_u, a.init_ring, ty0, tx0, a.H, a.W);
            if (a.init && !uni_init && !(TZW_ABL & 64)) {
                const float* initn = a.init + (long long)n * a.init_nstride;   // (0 for the per-model G0; a split launch's start values are per item)
                if (ty0 + 16 <= a.H && tx0 + 16 <= a.W) {   // (uniform) the whole tile inside the image: one lane offset, uniform steps
                    // (uniform) where G0 repeats tile by tile the reference tile stands in for this one (ConvArgs::init_tring):
                    // every workgroup of the launch then reads the same block
                    const bool rep = tile_uniform(a.init, a.init_tring, ty0, tx0, a.H, a.W);
                    const int yr = rep ? y - ty0 + ref_tile_origin(a.H) : y, xr = rep ? x0 - tx0 + ref_tile_origin(a.W) : x0;
                    const float* ip = initn + (unsigned)((yr * a.W + xr) * a.ncols + cb * CBW + r);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float* ie = ip + (unsigned)(2 * e * a.ncols);
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            in0[t][e] = ie[TZW_COLT(t)];
                            in1[t][e] = ie[a.ncols + TZW_COLT(t)];
                        }
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int col = cb * CBW + TZW_COLT(t) + r;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int x = x0 + 2 * e;
                            const bool ok = y < a.H && x < a.W;   // (W even wherever tiles are cut: x + 1 < W too)
                            const float* ip = initn + ((long long)(ok ? y * a.W + x : 0)) * a.ncols + col;
                            in0[t][e] = ip[0];
                            in1[t][e] = ip[x + 1 < a.W && ok ? a.ncols : 0];
                        }
                    }
                }
            } else {
                const float* bu = uni_init && !(TZW_ABL & 64) ? a.init_u : a.bias;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float b = bu[cb * CBW + TZW_COLT(t) + r];
                    in0[t] = in1[t] = (f32x4){b, b, b, b};
                }
            }
        }
        f32x4* xo = (f32x4*)(smem + TZW_XOFF) + (wv * 2) * 64 + lane;
        const f32x4* xi = (const f32x4*)(smem + TZW_XOFF) + ((wv ^ 4) * 2) * 64 + lane;
        if (NOSAME) {   // the chains as the launch over the same-resolution source left them
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                Y[0][t] = in0[t];
                Y[1][t] = in1[t];
            }
            // into their accumulation registers HERE, two wait states ahead of any MFMA that takes them as C (the asm MFMAs get
            // no hazard handling: a v_accvgpr_write sunk to right in front of the first stage would be read too early)
            static_assert(!NOSAME || EPI == EPI_LSTM || EPI == EPI_LSTM3, "the split launch exists for gate convolutions");
            if (NT == 4) asm volatile("" : "+a"(Y[0][0]), "+a"(Y[0][1]), "+a"(Y[0][2]), "+a"(Y[0][3]), "+a"(Y[1][0]), "+a"(Y[1][1]), "+a"(Y[1][2]), "+a"(Y[1][3]));
            else asm volatile("" : "+a"(Y[0][0]), "+a"(Y[0][1]), "+a"(Y[0][2]), "+a"(Y[1][0]), "+a"(Y[1][1]), "+a"(Y[1][2]));
            asm volatile("s_nop 1" ::: "memory");
        } else
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            constexpr int XA = XBYTES / 2 / 16;   // (f32x4 units) the second area
            const int xa = (t & 1) * XA;
            // (the accumulators of this round are read HERE: hoisted, they and the start values went through ~300 register
            // moves between VGPRs and AGPRs)
            asm volatile("" : "+a"(D[0][t]), "+a"(D[1][t]), "+a"(D[2][t]), "+a"(D[3][t]), "+a"(D[4][t]), "+a"(D[5][t]), "+a"(D[6][t]), "+a"(D[7][t]));
            // row sums of the wave's two transform rows
            const f32x4 za0 = (D[0][t] + D[1][t]) + D[2][t], za1 = (D[1][t] - D[2][t]) - D[3][t];
            const f32x4 zb0 = (D[4][t] + D[5][t]) + D[6][t], zb1 = (D[5][t] - D[6][t]) - D[7][t];
            if (ph == 0) {   // (uniform)
                xo[xa] = zb0;
                xo[xa + 64] = zb1;
            } else {
                xo[xa] = za0;
                xo[xa + 64] = za1;
            }
            if (!(TZW_ABL & 128)) __syncthreads();
            const f32x4 p0 = xi[xa], p1 = xi[xa + 64];
            if (ph == 0) {
                Y[0][t] = ((in0[t] + za0) + zb0) + p0;
                Y[1][t] = ((in1[t] + za1) + zb1) + p1;
            } else {
                Y[0][t] = ((in0[t] + p0) - za0) - zb0;
                Y[1][t] = ((in1[t] + p1) - za1) - zb1;
            }
        }
    }
