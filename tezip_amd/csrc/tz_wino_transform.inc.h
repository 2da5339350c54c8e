// k_wino / k_wino2 (tz_wino_kernels.hip.h), a section of the kernel body both share as text: the patch reads of a wave and B^T d B.
    auto read_d = [&](unsigned ad, f32x2 (&d)[3][2]) {
        read_rows<0>(ad, d);
        read_rows<1>(ad, d);
        read_rows<2>(ad, d);
    };
    // B^T d B for the wave's two transform rows (same association as the oracle): columns first, then rows
    auto transform = [&](const f32x2 (&d)[3][2], float (&V)[8]) {
#if TZW_PK
        // 10 packed instructions instead of 20: per row T1 = (t0, t3) = (d0, d1) - (d2, d3), T2 = (t1, t2) = (d1 + d2, d2 - d1);
        // then the rows the same way on the pairs
        f32x2 T1[3], T2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            T1[k] = pk_sub(d[k][0], d[k][1]);
            T2[k] = pk_cross(d[k][0], d[k][1]);
        }
        f32x2 a03, a12, b03, b12;   // (V[.][0], V[.][3]), (V[.][1], V[.][2]) of the wave's two transform rows
        if (ph == 0) {   // rows 0, 1, 2 of the patch: V[0] = t0 - t2, V[1] = t1 + t2
            a03 = pk_sub(T1[0], T1[2]);
            a12 = pk_sub(T2[0], T2[2]);
            b03 = pk_add(T1[1], T1[2]);
            b12 = pk_add(T2[1], T2[2]);
        } else {         // rows 1, 2, 3: V[2] = t2 - t1, V[3] = t1 - t3
            a03 = pk_sub(T1[1], T1[0]);
            a12 = pk_sub(T2[1], T2[0]);
            b03 = pk_sub(T1[0], T1[2]);
            b12 = pk_sub(T2[0], T2[2]);
        }
        V[0] = a03[0]; V[3] = a03[1]; V[1] = a12[0]; V[2] = a12[1];
        V[4] = b03[0]; V[7] = b03[1]; V[5] = b12[0]; V[6] = b12[1];
        return;
#endif
        float t[3][4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float d0 = d[k][0][0], d2 = TZW_PK ? d[k][1][0] : d[k][0][1], d1 = TZW_PK ? d[k][0][1] : d[k][1][0], d3 = d[k][1][1];
            t[k][0] = fsub(d0, d2);
            t[k][1] = fadd(d1, d2);
            t[k][2] = fsub(d2, d1);
            t[k][3] = fsub(d1, d3);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (ph == 0) {   // rows 0, 1, 2 of the patch: V[0] = t0 - t2, V[1] = t1 + t2
                V[j] = fsub(t[0][j], t[2][j]);
                V[4 + j] = fadd(t[1][j], t[2][j]);
            } else {         // rows 1, 2, 3: V[2] = t2 - t1, V[3] = t1 - t3
                V[j] = fsub(t[1][j], t[0][j]);
                V[4 + j] = fsub(t[0][j], t[2][j]);
            }
        }
    };
