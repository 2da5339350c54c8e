// k_wino / k_wino2 (tz_wino_kernels.hip.h), a section of the kernel body both share as text: the fused epilogues of an item.
    // ---- epilogues.  This wave's outputs: pixel row a = ph of its 16 tiles, columns b = 0, 1: Y[b][column tile][e],
    // accumulator row 4 g + e = tile (tyl = g, txl = e)
    const int oy = ty0 + 8 * (mt >> 1) + 2 * g + ph + per_item;
    if (EPI == EPI_RAW || EPI == EPI_RAW3) {
        // (EPI_RAW3: the rows written are 3 Cout wide -- [i | g | o] x 16 per block --, the rows of the start values 4 Cout = a.ncols)
        const int ocols = EPI == EPI_RAW3 ? 3 * a.Cout : a.ncols;
        float* on = a.out0 + (long long)n * a.out0_nstride;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int x = tx0 + 8 * (mt & 1) + 2 * e + b;
                if (oy < a.H && x < a.W) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) on[((long long)oy * a.W + x) * ocols + cb * (16 * NT) + 16 * t + r] = Y[b][t][e];
                }
            }
    } else if (EPI == EPI_LSTM || EPI == EPI_LSTM3) {
        // columns of this block: [i | f | g | o] x 16 channels of channel group cb (prednet.py:255-259):
        // c = f * c_prev + i * g ; r = o * tanh(c)
        // EPI_LSTM3: [i | g | o], c_prev = +0 everywhere: f * (+0) = +0 for every non-NaN f, so c = (+0) + i * g -- a real
        // float32 addition (it turns i * g = -0 into +0, as the four-gate form does), no cell state is loaded
        constexpr bool F3 = EPI == EPI_LSTM3;
        constexpr int TG = F3 ? 1 : 2 % NT, TO = F3 ? 2 : 3 % NT;   // column tiles of gates g and o
        const int ch = cb * 16 + r, R = a.Cout;
        float* o0 = a.out0 + (long long)n * a.out0_nstride;
        float* o1 = a.out1 ? a.out1 + (long long)n * a.out1_nstride : nullptr;
        if (ty0 + 16 <= a.H && tx0 + 16 <= a.W && !(TZW_ABL & 512)) {
            // (uniform) the whole tile inside the image: ONE lane offset for the eight outputs of a lane, the steps between
            // them uniform -- scalar base + 32-bit lane offset addressing, no per-output predicates (the general form below
            // spends ~25 instructions per output on 64-bit addresses and exec masks; in a serial section, with the matrix
            // pipes idle, instructions are what costs)
            const unsigned voff = 4u * (unsigned)((oy * a.W + tx0 + 8 * (mt & 1)) * R + ch);
            const char* pc = (const char*)a.aux;
            char* p0 = (char*)o0;
            char* p1 = (char*)o1;
            float cpv[2][4];
            if (F3) {
                // (no cell state to load)
            } else if (tile_uniform(a.aux_u, a.aux_ring, ty0, tx0, a.H, a.W) && !(TZW_ABL & 256)) {
                // (uniform) away from the border of the plane the cell state is one value per channel: one load
                const float cu = a.aux_u[ch];
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int e = 0; e < 4; ++e) cpv[b][e] = cu;
            } else {
                // (uniform) where the cell state repeats tile by tile: the reference tile's values (ConvArgs::aux_tring)
                const unsigned roff = 4u * (unsigned)(((ref_tile_origin(a.H) - ty0) * a.W + ref_tile_origin(a.W) - tx0) * R);
                const unsigned coff = tile_uniform(a.aux, a.aux_tring, ty0, tx0, a.H, a.W) ? voff + roff : voff;
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        cpv[b][e] = a.aux && !(TZW_ABL & 256) ? *(const float*)(pc + (size_t)(2 * e + b) * R * 4 + coff) : 0.0f;
            }
#ifdef TZW_STAMPS
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            TZW_STAMP(6)
#endif
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float gi = tz_hard_sigmoid(Y[b][0][e]);
                    const float gg = tz_tanh(Y[b][TG][e]);
                    const float go = tz_hard_sigmoid(Y[b][TO][e]);
                    const float t2 = gi * gg;
                    float c;
                    if (F3) {
                        c = fadd_zero(t2);
                    } else {
                        const float gf = tz_hard_sigmoid(Y[b][1 % NT][e]);
                        const float t1 = gf * cpv[b][e];
                        c = t1 + t2;
                    }
                    const float rr = go * tz_tanh(c);
                    *(float*)(p0 + (size_t)(2 * e + b) * R * 4 + voff) = rr;
                    if (o1) *(float*)(p1 + (size_t)(2 * e + b) * R * 4 + voff) = c;
                }
        } else {
        long long pix[2][4];
        bool ok[2][4];
        float cp[2][4];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int x = tx0 + 8 * (mt & 1) + 2 * e + b;
                ok[b][e] = oy < a.H && x < a.W;
                pix[b][e] = ok[b][e] ? (long long)oy * a.W + x : 0;
                // (Asking for these ahead of the output transform through asm loads -- to hide their round trip -- is NOT
                // safe: the compiler is free to reuse an asm load's destination register before the data lands, and did:
                // the late write then hit an address register, a memory fault in the bench.  Plain loads, at their use.)
                cp[b][e] = !F3 && a.aux && !(TZW_ABL & 256) ? a.aux[pix[b][e] * R + ch] : 0.0f;
            }
#ifdef TZW_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        TZW_STAMP(6)
#endif
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (TZW_ABL & 512) {
                    if (ok[b][e]) {
                        o0[pix[b][e] * R + ch] = Y[b][0][e] + Y[b][1 % NT][e] + cp[b][e];
                        if (o1) o1[pix[b][e] * R + ch] = Y[b][2 % NT][e] + Y[b][3 % NT][e];
                    }
                    continue;
                }
                const float gi = tz_hard_sigmoid(Y[b][0][e]);
                const float gg = tz_tanh(Y[b][TG][e]);
                const float go = tz_hard_sigmoid(Y[b][TO][e]);
                const float t2 = gi * gg;
                float c;
                if (F3) {
                    c = fadd_zero(t2);
                } else {
                    const float gf = tz_hard_sigmoid(Y[b][1 % NT][e]);
                    const float t1 = gf * cp[b][e];
                    c = t1 + t2;
                }
                const float rr = go * tz_tanh(c);
                if (ok[b][e]) {
                    o0[pix[b][e] * R + ch] = rr;
                    if (o1) o1[pix[b][e] * R + ch] = c;
                }
            }
        }
    } else if (EPI == EPI_POOL_ERR) {
        // prednet.py:289-291 then 274-277 of the next level: A = maxpool2x2(relu(conv)) -- the pooling window IS the tile --,
        // e = [relu(Ahat0 - A), relu(A - Ahat0)] at the pooled resolution.  The wave holds one row of every window; the
        // partner the other: wave ph = 0 finishes column tiles 0, 1, wave ph = 1 the rest
        // (ConvArgs::dead_half: Ahat0 is +-0 over the plane -- no load of it, no subtraction, the live half A alone stored)
        const int H2 = a.H >> 1, W2 = a.W >> 1, C = a.Cout;
        float* o = a.out0 + (long long)n * a.out0_nstride;
        f32x4 m[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v0 = tz_relu(Y[0][t][e]), v1 = tz_relu(Y[1][t][e]);
                m[t][e] = v1 > v0 ? v1 : v0;
            }
        // (the exchange area the last round of the output transform did NOT use: a partner may still be reading that one)
        constexpr int XP = (NT & 1) * (XBYTES / 2 / 16);
        f32x4* xo = (f32x4*)(smem + TZW_XOFF) + XP + (wv * 2) * 64 + lane;
        const f32x4* xi = (const f32x4*)(smem + TZW_XOFF) + XP + ((wv ^ 4) * 2) * 64 + lane;
        // (no run-time indices into m[]: it has to stay in registers)
        xo[0] = ph == 0 ? m[2] : m[0];                       // the column tiles the partner finishes
        xo[64] = ph == 0 ? m[NT - 1] : m[1];                 // (NT = 3: the second one of wave 0 is not used)
        __syncthreads();
        const f32x4 q0 = xi[0], q1 = xi[64];
        const int yp = (ty0 >> 1) + 4 * (mt >> 1) + g + per_item;
        if (ty0 + 16 <= a.H && tx0 + 16 <= a.W && (cb + 1) * (16 * NT) <= C && !(TZW_ABL & 512)) {
            // (uniform) the whole tile inside the image and the whole column block inside the stack: ONE lane offset per
            // array for the outputs of a lane, uniform steps between them -- scalar base + 32-bit lane offset addressing, no
            // per-output predicates (what the LSTM epilogue got in round 4; the general form below spends ~25 instructions
            // per output on 64-bit addresses and exec masks, in a serial section with the matrix pipes idle)
            const unsigned pix = (unsigned)(yp * W2 + (tx0 >> 1) + 4 * (mt & 1));
            const unsigned colw = (unsigned)(cb * (16 * NT) + r);
            const char* ph_ = (const char*)a.aux;
            char* po = (char*)o;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (ph == 1 && 2 + k >= NT) break;
                const int t = (ph == 0 ? 0 : 2) + k;
                const f32x4 mine = ph == 0 ? m[k] : m[(2 + k) % NT], other = k == 0 ? q0 : q1;
                const unsigned hoff = 4u * (pix * (unsigned)C + colw + 16u * t), ooff = 4u * (pix * 2u * (unsigned)C + colw + 16u * t);
                if (a.dead_half) {   // (uniform) Ahat0 = +-0 over the plane and mm >= +0: e = [+0 | mm], the +0 is there already
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float mm = other[e] > mine[e] ? other[e] : mine[e];
                        *(float*)(po + (size_t)e * C * 8 + (size_t)C * 4 + ooff) = mm;
                    }
                    continue;
                }
                float hv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[e] = *(const float*)(ph_ + (size_t)e * C * 4 + hoff);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float mm = other[e] > mine[e] ? other[e] : mine[e];
                    const float d1 = hv[e] - mm, d2 = mm - hv[e];
                    *(float*)(po + (size_t)e * C * 8 + ooff) = tz_relu(d1);
                    *(float*)(po + (size_t)e * C * 8 + (size_t)C * 4 + ooff) = tz_relu(d2);
                }
            }
        } else
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (ph == 1 && 2 + k >= NT) break;               // wave 1 finishes column tiles 2 .. NT - 1, wave 0 tiles 0, 1
            const int t = (ph == 0 ? 0 : 2) + k;
            const f32x4 mine = ph == 0 ? m[k] : m[(2 + k) % NT], other = k == 0 ? q0 : q1;
            const int ch = cb * (16 * NT) + 16 * t + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int xp = (tx0 >> 1) + 4 * (mt & 1) + e;
                const bool okp = yp < H2 && xp < W2 && ch < C;
                const long long pp = okp ? (long long)yp * W2 + xp : 0;
                const float mm = other[e] > mine[e] ? other[e] : mine[e];
                if (a.dead_half) {   // (uniform)
                    if (okp) o[pp * 2 * C + C + ch] = mm;
                    continue;
                }
                const float h = a.aux[okp ? pp * C + ch : 0];
                const float d1 = h - mm, d2 = mm - h;
                if (okp) {
                    o[pp * 2 * C + ch] = tz_relu(d1);
                    o[pp * 2 * C + C + ch] = tz_relu(d2);
                }
            }
        }
    }
