    // The statements of t5_attention_kernel<D> / lm_causal_attention_kernel<D>, included inside the kernel after
    // `typedef ... Policy;` with the kernel argument named p (text_attn_tile.h says what a policy is, and why this is no function).
    __shared__ float qs[TA_QT][D];
    __shared__ float ks[TA_KT][D + 1];
    __shared__ float vs[TA_KT][D];
    __shared__ float ps[TA_WAVES][TA_KT];
    __shared__ int ms[TA_KT];
    constexpr int G = 64 / D;               // key groups of the P.V product
    constexpr int D4 = D / 4;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int qt = blockIdx.x % p.qtiles;
    const int h = (blockIdx.x / p.qtiles) % p.H;
    const int b = blockIdx.x / (p.qtiles * p.H);
    const Policy pol(p, b, h, D);
    const int i0 = qt * TA_QT, Nq = pol.rows, Nk = pol.nkeys;

    for (int e = tid; e < TA_QT * D4; e += 64 * TA_WAVES) {
        const int r = e / D4, c = e - r * D4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i0 + r < Nq) a = ((const float4*)(pol.q + (size_t)(i0 + r) * (size_t)pol.ldq))[c];
        qs[r][4 * c] = a.x; qs[r][4 * c + 1] = a.y; qs[r][4 * c + 2] = a.z; qs[r][4 * c + 3] = a.w;
    }
    float m[TA_RPW], l[TA_RPW], acc[TA_RPW];
#pragma unroll
    for (int rr = 0; rr < TA_RPW; ++rr) { m[rr] = -INFINITY; l[rr] = 0.f; acc[rr] = 0.f; }
    const int g = lane / D, d = lane - g * D;
    const int jend = pol.key_end(i0);

    for (int j0 = 0; j0 < jend; j0 += TA_KT) {
        __syncthreads();                                    // the previous tile's readers are done (first pass: nothing pending)
        for (int e = tid; e < TA_KT * D4; e += 64 * TA_WAVES) {
            const int r = e / D4, c = e - r * D4;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), bb = a;
            if (j0 + r < Nk) {
                a = ((const float4*)(pol.k + (size_t)(j0 + r) * (size_t)pol.ldk))[c];
                bb = ((const float4*)(pol.v + (size_t)(j0 + r) * (size_t)pol.ldv))[c];
            }
            ks[r][4 * c] = a.x; ks[r][4 * c + 1] = a.y; ks[r][4 * c + 2] = a.z; ks[r][4 * c + 3] = a.w;
            vs[r][4 * c] = bb.x; vs[r][4 * c + 1] = bb.y; vs[r][4 * c + 2] = bb.z; vs[r][4 * c + 3] = bb.w;
        }
        if (tid < TA_KT) ms[tid] = (j0 + tid < Nk) && (pol.mask == nullptr || pol.mask[j0 + tid] != 0);
        __syncthreads();
        const bool live = ms[lane] != 0;
#pragma unroll
        for (int rr = 0; rr < TA_RPW; ++rr) {
            const int r = wave * TA_RPW + rr, i = i0 + r;
            if (i >= Nq) continue;                          // (wave-uniform)
            if (pol.skip(i, j0)) continue;                  // (wave-uniform)
            const bool valid = pol.valid(live, i, j0 + lane);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
            for (int dd = 0; dd < D; dd += 4) {
                s0 = fmaf(qs[r][dd], ks[lane][dd], s0);
                s1 = fmaf(qs[r][dd + 1], ks[lane][dd + 1], s1);
                s2 = fmaf(qs[r][dd + 2], ks[lane][dd + 2], s2);
                s3 = fmaf(qs[r][dd + 3], ks[lane][dd + 3], s3);
            }
            float sc = -INFINITY;
            if (valid) sc = pol.score((s0 + s1) + (s2 + s3), i, j0 + lane);
            const float mt = aed_wave_max(sc);
            if (mt == -INFINITY) continue;                  // no attended key in this tile (wave-uniform)
            const float mn = fmaxf(m[rr], mt);
            const float alpha = expf(m[rr] - mn);           // first attended tile: exp(-inf) = 0
            const float pj = valid ? expf(sc - mn) : 0.f;
            l[rr] = l[rr] * alpha + aed_wave_sum(pj);
            m[rr] = mn;
            __builtin_amdgcn_wave_barrier();                // the previous row's reads of ps[wave] are issued (LDS is in order)
            ps[wave][lane] = pj;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            float a = 0.f;
#pragma unroll 8
            for (int jj = 0; jj < TA_KT / G; ++jj) a = fmaf(ps[wave][jj * G + g], vs[jj * G + g][d], a);
            acc[rr] = acc[rr] * alpha + a;
        }
    }
#pragma unroll
    for (int rr = 0; rr < TA_RPW; ++rr) {
        const int i = i0 + wave * TA_RPW + rr;
        if (i >= Nq) continue;
        float a = acc[rr];
#pragma unroll
        for (int o = D; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
        if (lane < D) pol.out[(size_t)i * (size_t)pol.ldo + lane] = l[rr] > 0.f ? a / l[rr] : 0.f;
    }
