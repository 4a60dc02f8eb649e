// kid_tile_loop.h - the loop of one workgroup of kid.hip's tile-sum kernels, included as TEXT into the body of each of them (no include guard:
// it is included twice).  A forceinline function would serve the grouped kernel as well, but moves the pooled kernel's register allocation
// (157 -> 153 VGPRs, measured); as text the pooled kernel is token for token what it was, and both kernels run one and the same loop.
// The including kernel has in scope: a, m, b, n, d, gamma, coef0, exclude_diag, vec4, slab, sums - the operands, counts and row-major tile
// matrix [ceil(m / 64), ceil(n / 64)] of THIS workgroup's problem (the grouped kernel has moved them to its class's segment) - and defines
//   KID_BLK   the tile of 64 rows of a this workgroup owns            KID_SLAB  which slab of `slab` consecutive tiles of b it sums
// as expressions that name nothing this text declares (tid, wave, lane, lc, lq, row0, arow, ap, nchunk, ntile, tile0, tile1, tile, ...).
    __shared__ __attribute__((aligned(16))) float stage[TN][LDB];
    __shared__ double wsum[WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const long long row0 = KID_BLK * TM + 16 * wave;
    const long long arow = row0 + lc;                   // the row of a this lane loads as the A operand
    const bool arow_ok = arow < m;
    const float* ap = a + (arow_ok ? arow : m - 1) * d;      // a row past m reads the last one and is masked

    const int nchunk = (d + DK - 1) / DK;
    const long long ntile = (n + TN - 1) / TN;
    const long long tile0 = KID_SLAB * slab;
    const long long tile1 = tile0 + slab < ntile ? tile0 + slab : ntile;      // the host launches no empty slab: tile0 < ntile
    // the next chunk in registers: float4 e = tid + TPB u of the [TN][DK / 4] chunk of b (a row of the chunk per 16 lanes) and this lane's A
    // operands of the chunk's 16 steps.  A chunk wholly inside b, with 16-byte aligned rows, is loaded without a test per element.
    float pre[PRE], apre[DK / 4], acur[DK / 4];
    auto fetch = [&](long long tile, int c) {
        const bool k_full = (c + 1) * DK <= d;
        if (vec4 && k_full && (tile + 1) * TN <= n) {
            const float* src = b + (tile * TN + (tid >> 4)) * d + c * DK + 4 * (tid & 15);
#pragma unroll
            for (int u = 0; u < PRE / 4; ++u) {
                const float4 v = *reinterpret_cast<const float4*>(src + (long long)(TPB / 16) * u * d);
                pre[4 * u] = v.x, pre[4 * u + 1] = v.y, pre[4 * u + 2] = v.z, pre[4 * u + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int u = 0; u < PRE; ++u) {
                const int e = tid + TPB * (u / 4);
                const long long j = tile * TN + (e >> 4);
                const int kg = c * DK + 4 * (e & 15) + (u & 3);
                pre[u] = (j < n && kg < d) ? b[j * d + kg] : 0.f;
            }
        }
        if (k_full) {
#pragma unroll
            for (int u = 0; u < DK / 4; ++u) apre[u] = ap[c * DK + 4 * u + lq];
        } else {
#pragma unroll
            for (int u = 0; u < DK / 4; ++u) {
                const int kg = c * DK + 4 * u + lq;
                apre[u] = kg < d ? ap[kg] : 0.f;
            }
        }
    };
    fetch(tile0, 0);
    for (long long tile = tile0; tile < tile1; ++tile) {
        double4_t acc[SUB];
#pragma unroll
        for (int s = 0; s < SUB; ++s) acc[s] = double4_t{0., 0., 0., 0.};
        for (int c = 0; c < nchunk; ++c) {
            __syncthreads();      // the previous chunk's reads (and the previous tile's read of wsum) are done
#pragma unroll
            for (int u = 0; u < PRE / 4; ++u) {
                const int e = tid + TPB * u;
                *reinterpret_cast<float4*>(&stage[e >> 4][4 * (e & 15)]) = make_float4(pre[4 * u], pre[4 * u + 1], pre[4 * u + 2], pre[4 * u + 3]);
            }
#pragma unroll
            for (int u = 0; u < DK / 4; ++u) acur[u] = arow_ok ? apre[u] : 0.f;
            __syncthreads();
            if (c + 1 < nchunk) fetch(tile, c + 1);
            else if (tile + 1 < tile1) fetch(tile + 1, 0);
            const int left = d - c * DK;      // a step past d adds exactly 0 and may be left out
#pragma unroll
            for (int u = 0; u < DK / 4; ++u) {
                if (4 * u < left) {
                    const int kk = 4 * u;
                    const double av = (double)acur[u];
                    double bv[SUB];
#pragma unroll
                    for (int s = 0; s < SUB; ++s) bv[s] = (double)stage[16 * s + lc][kk + lq];
#pragma unroll
                    for (int s = 0; s < SUB; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[s], acc[s], 0, 0, 0);
                }
            }
        }

        // this lane's 16 kernel values, masked by index, in the order (C tile, register)
        const long long jt = tile * TN;
        double part = 0.;
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
            const long long j = jt + 16 * s + lc;
            const bool j_ok = j < n;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long i = row0 + lq + 4 * r;
                const double v = gamma * acc[s][r] + coef0;
                const double k3 = (v * v) * v;
                const bool keep = j_ok && i < m && !(exclude_diag && i == j);
                part += keep ? k3 : 0.;
            }
        }
        // the wave's 64 lanes: every lane ends with the same sum; then the four waves in order
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off, 64);
        if (lane == 0) wsum[wave] = part;
        __syncthreads();
        if (tid == 0) sums[KID_BLK * ntile + tile] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
