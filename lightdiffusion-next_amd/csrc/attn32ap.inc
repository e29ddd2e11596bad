// Included by attention.hip (inside namespace ldx, after attn32_kernel).
// ------------------------------------------------------------------------------------------------------------
// Round 3: 8-wave ANTI-PHASE form of attn32_kernel for the step's largest launches (D = 40, N = 16384; Attention.py:100-124 through
// AttentionMethods.py:107-150).  In attn32_kernel the two waves of a SIMD (one from each of the CU's two 4-wave workgroups) free-run
// through the same phase-structured loop; the matrix pipe and the VALU then serve them one after the other (profiles/ubench/antiphase.hip:
// blocked 1938 nominal cycles per wave-iteration, barrier-enforced anti-phase 1626-1671, VALU floor ~1300).  Here ONE 512-thread workgroup
// owns the CU: waves 0-3 (group 0) and 4-7 (group 1) — one of each per SIMD — run the same per-block sequence
//     M(i) = { PV(i-1), QK^T(i), staging }   /   V(i) = { V^T fragment prefetch, online softmax -> P(i) }
// one PHASE apart, with one s_barrier per phase: while group 0 issues MFMAs, group 1 runs its softmax on the VALU, then the roles swap.
//   phase t:   0      1      2      3      4     ...
//   group 0:  M(0)   V(0)   M(1)   V(1)   M(2)
//   group 1:   -     M(0)   V(0)   M(1)   V(1)
// K/V tiles are shared by all 512 queries of the workgroup (half the staging work per query).  K(j) is read in phases 2j (g0) and 2j+1
// (g1), V(j) in 2j+1 and 2j+2; the staging stores ride in the MFMA phases, which have slack (28 MFMAs ~ 900 cycles against ~1300 of
// softmax): group 1 writes K(i+1) in its M(i) (phase 2i+1: slot (i+1)&1 was last read in phase 2i-1), group 0 writes V(i) in its M(i)
// (phase 2i: slot i&1 was last read in phase 2i-2); each group's global loads for its next tile are issued right after the store, a
// whole two-phase period ahead of their use.  Arithmetic, operand layouts and LDS strides are attn32_kernel's: same results bit for bit.
template <typename T, int KROWB, int VROWB, int VAR>
__global__ __launch_bounds__(512, 1) void attn32ap_kernel(const AttnArgs p) {
    constexpr int QW = 64, QB = 512, KVB = 64;
    constexpr int KBYTES = KVB * KROWB, VBYTES = KVB * VROWB;
    static_assert(KROWB == A32_KROW && VROWB == A32_VROW && 2 * (KBYTES + VBYTES) == attn32_lds(KVB), "attn_pick (attn_pick.cpp) plans with these strides");
    extern __shared__ __attribute__((aligned(16))) char smem[];       // K ring [2][KBYTES] | V ring [2][VBYTES]
    using V8 = typename Vec<T>::v8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = wave >> 2;                                            // waves w and w + 4 share a SIMD
    const int l31 = lane & 31, h2 = lane >> 5, l15 = lane & 15, g16 = lane >> 4;
    const int nqb = (p.Nq + QB - 1) / QB;
    const int lin = xcd_remap(blockIdx.x, nqb * p.H * p.B);
    const int qblk = lin % nqb, hb = lin / nqb;
    const int h = hb % p.H, b = hb / p.H;
    const int q0 = qblk * QB + wave * QW;
    const int D = p.D, dch = D >> 3;
    const T* __restrict__ Qp = (const T*)p.Q + (long)b * p.Nq * p.ldq + h * D;
    const T* __restrict__ Kp = (const T*)p.K + (long)b * p.Mk * p.ldk + h * D;
    const T* __restrict__ Vp = (const T*)p.V + (long)b * p.Mk * p.ldv + h * D;
    T* __restrict__ Op = (T*)p.O + (long)b * p.Nq * p.ldo + h * D;
    const float c = p.scale * 1.44269504088896340736f;

    for (int i = tid; i < (2 * (KBYTES + VBYTES)) / 16; i += 512) *(uint4*)(smem + i * 16) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    if (tid < 2 * KVB) *(T*)(smem + 2 * KBYTES + (tid >> 6) * VBYTES + (tid & 63) * VROWB + D * 2) = (T)1.0f;       // ones column of V at d = D

    V8 qf[2][3];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + qt * 32 + l31;
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
            const int ch = 2 * ks + h2;
            uint4 u = make_uint4(0, 0, 0, 0);
            if (q < p.Nq && ch < dch) u = *(const uint4*)(Qp + (long)q * p.ldq + ch * 8);
            asm volatile("" : "+v"(u.x), "+v"(u.y), "+v"(u.z), "+v"(u.w));      // wait for Q here, not inside the loop (see attn32_kernel)
            qf[qt][ks] = as_v8<T>(u);
        }
    }
    f32x16 o[2][2];
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    o[0][0] = zero16; o[0][1] = zero16; o[1][0] = zero16; o[1][1] = zero16;
    float mrun[2] = {-INFINITY, -INFINITY};
    const int nblk = (p.Mk + KVB - 1) / KVB;

    // staging: group 1 moves the K tiles, group 0 the V tiles (256 threads per 64 x D tile, up to 2 chunks of 16 B per thread)
    constexpr int OOB = (int)0x80000000;
    // VAR & 128 (K fragments read a phase early): the staging roles are swapped — group 0 writes K(i+1) in its M(i) (phase 2i), group 1 writes
    // V(i+1) in its M(i) (phase 2i+1) — so that K(i+1) is visible one phase before either group's M(i+1) and its six fragments can be read
    // during V(i), next to the V^T fragments: the matrix phase then starts on its MFMAs instead of on an exposed LDS round trip.
    constexpr bool KPRE = (VAR & 128) != 0;
    const bool gk = KPRE ? (g == 0) : (g != 0);                     // this group stages K (else V)
    const int ld_g = gk ? p.ldk : p.ldv;
    const __amdgpu_buffer_rsrc_t rG = __builtin_amdgcn_make_buffer_rsrc((void*)(gk ? Kp : Vp), 0, (int)(((long)(p.Mk - 1) * ld_g + D) * 2), RSRC_RAW_WORD3);
    char* const ringG = smem + (gk ? 0 : 2 * KBYTES);
    const int rowb_g = gk ? KROWB : VROWB, tileb_g = gk ? KBYTES : VBYTES;
    uint4 rs[2];
    int go[2], lo[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = (tid & 255) + i * 256;
        const int row = idx / dch, ch = idx - row * dch;
        const bool in_tile = row < KVB;
        go[i] = in_tile ? (row * ld_g + ch * 8) * 2 : OOB;
        lo[i] = in_tile ? row * rowb_g + ch * 16 : -1;
    }
    const int gstep = KVB * ld_g * 2;
    auto gload = [&](int blk) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const auto a = __builtin_amdgcn_raw_buffer_load_b128(rG, go[i] != OOB ? go[i] + blk * gstep : OOB, 0, 0);
            rs[i] = make_uint4(a[0], a[1], a[2], a[3]);
        }
    };
    auto lstore = [&](int blk) __attribute__((always_inline)) {
        char* sB = ringG + (blk & 1) * tileb_g;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (lo[i] >= 0) *(uint4*)(sB + lo[i]) = rs[i];
    };

    __syncthreads();
    if (KPRE || g) { gload(0); lstore(0); if (nblk > 1) gload(1); }       // K(0) in place, K(1) in flight (KPRE: V(0) / V(1) as well)
    else gload(0);                                                  // V(0) in flight: written in group 0's M(0)
    __syncthreads();
    if (g) __builtin_amdgcn_s_barrier();                            // group 1 runs one phase behind

    f32x16 s[2][2];                                                 // S^T of a block between its M and V phases
    V8 pf[2][4];                                                    // P^T of the previous block (B operand of PV)
    V8 vpre[4][2];                                                  // ... and its V^T fragments
    // The sequence is peeled (M(0) | { V(i), M(i+1) } x (nblk-1) | V(nblk-1), M(nblk)) so that s / pf / vpre are defined unconditionally in
    // every loop iteration: as conditionally-defined loop-carried values they were all live across the back edge and spilled (504 B of scratch).
    auto pv = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) o[qt][dt] = mfma32(vpre[st][dt], pf[qt][st], o[qt][dt]);
    };
    // VAR & 64 (split softmax): the V phase only produces P^T of the block's first 32 keys; the exponentials of the other 32 ride in the NEXT
    // matrix phase of the same wave, pinned between the PV MFMAs of the first half (a wave's own VALU work issues in the shadow of its own MFMAs;
    // VALU work of the SIMD's other wave does not — profiles/ubench/pipes.hip).  Same arithmetic in the same order per element: same bits.
    constexpr bool SPLIT = (VAR & 64) != 0;
    float mcs[2] = {0.f, 0.f};                                      // running maximum * c of the block in flight, per query tile
    auto exp4 = [&](int qt, int st, int e0) __attribute__((always_inline)) {
#pragma unroll
        for (int e = e0; e < e0 + 4; ++e) pf[qt][st][e] = (T)__builtin_amdgcn_exp2f(fmaf(s[st >> 1][qt][8 * (st & 1) + e], c, -mcs[qt]));
    };
    auto pv_split = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {                               // PV of keys 0..31 (st 0, 1), four independent accumulators in turn
            const int st = m >> 2, dt = (m >> 1) & 1, qt = m & 1;
            o[qt][dt] = mfma32(vpre[st][dt], pf[qt][st], o[qt][dt]);
            exp4(m >> 2, 2 + ((m >> 1) & 1), 4 * (m & 1));          // ... and 4 of the 32 deferred exponentials behind each of them
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int st = 2; st < 4; ++st)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) o[qt][dt] = mfma32(vpre[st][dt], pf[qt][st], o[qt][dt]);
    };
    auto stage = [&](int i) __attribute__((always_inline)) {
        const int st = KPRE ? i + 1 : i + g;                        // group 0: V(i), group 1: K(i+1); KPRE: K(i+1) / V(i+1)
        if (st < nblk) lstore(st);
        if (st + 1 < nblk) gload(st + 1);
    };
    // M(i): PV(i-1) (PV = true), QK^T(i), staging
    V8 kf[3][2];
    auto kread = [&](int i) __attribute__((always_inline)) {
        const char* sK = smem + (i & 1) * KBYTES;
#pragma unroll
        for (int ks = 0; ks < 3; ++ks)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) kf[ks][kt] = as_v8<T>(*(const uint4*)(sK + (kt * 32 + l31) * KROWB + (2 * ks + h2) * 16));
    };
    auto mphase = [&](int i, auto PV) __attribute__((always_inline)) {
        if (!KPRE || !decltype(PV)::value) kread(i);
        if (VAR & 1) __builtin_amdgcn_s_setprio(1);
        if constexpr (decltype(PV)::value) { if (!(VAR & 4)) { if constexpr (SPLIT) pv_split(); else pv(); } }
        s[0][0] = zero16; s[0][1] = zero16; s[1][0] = zero16; s[1][1] = zero16;
#pragma unroll
        for (int ks = 0; ks < 3; ++ks)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) { if (!(VAR & 4)) s[kt][qt] = mfma32(kf[ks][kt], qf[qt][ks], s[kt][qt]); else { s[kt][qt][0] += (float)kf[ks][kt][0]; asm volatile("" : "+v"(s[kt][qt])); } }
        if (VAR & 1) __builtin_amdgcn_s_setprio(0);
        stage(i);
    };
    // V(i): V^T fragments of block i, online softmax
    auto vphase = [&](int i) __attribute__((always_inline)) {
        const char* sV = smem + 2 * KBYTES + (i & 1) * VBYTES;
        const int kv0 = i * KVB;
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const char* vp = sV + (16 * st + 4 * (g16 >> 1) + (l15 >> 2)) * VROWB + (dt * 32 + 16 * (g16 & 1) + (l15 & 3) * 4) * 2;
                U128 vf;
                vf.d[0] = lds_read_tr16(vp);
                vf.d[1] = lds_read_tr16(vp + 8 * VROWB);
                if (!(VAR & 16)) vpre[st][dt] = as_v8<T>(vf.u);
            }
        if (KPRE && i + 1 < nblk) kread(i + 1);
        if (VAR & 8) {        // ablation: no softmax
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int st = 0; st < 4; ++st)
#pragma unroll
                    for (int e = 0; e < 8; ++e) pf[qt][st][e] = (T)s[st >> 1][qt][8 * (st & 1) + e];
            return;
        }
        if constexpr (SPLIT) {
            if (kv0 + 64 > p.Mk) {                   // ragged last key block (wave-uniform branch), in place: the deferred half reads s again
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kv = kv0 + kt * 32 + 8 * (r >> 2) + 4 * h2 + (r & 3);
                        if (kv >= p.Mk) { s[kt][0][r] = -INFINITY; s[kt][1][r] = -INFINITY; }
                    }
                asm volatile("" ::: "memory");
            }
            float al[2];
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                float mx = max32_tree_v(s[0][qt], s[1][qt]);
                auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
                mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
                const float mnew = fmaxf(mrun[qt], mx);
                mcs[qt] = (mnew == -INFINITY) ? 0.f : mnew * c;
                al[qt] = __builtin_amdgcn_exp2f(mrun[qt] * c - mcs[qt]);
                mrun[qt] = mnew;
            }
            if (__builtin_amdgcn_ballot_w64(al[0] != 1.0f || al[1] != 1.0f) != 0) {
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) { o[qt][0] = o[qt][0] * al[qt]; o[qt][1] = o[qt][1] * al[qt]; }
            }
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int st = 0; st < 2; ++st) { exp4(qt, st, 0); exp4(qt, st, 4); }
            return;
        }
        float sv[2][2][16];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int r = 0; r < 16; ++r) sv[kt][qt][r] = s[kt][qt][r];
        if (kv0 + 64 > p.Mk) {                       // ragged last key block (wave-uniform branch)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kv = kv0 + kt * 32 + 8 * (r >> 2) + 4 * h2 + (r & 3);
                    if (kv >= p.Mk) { sv[kt][0][r] = -INFINITY; sv[kt][1][r] = -INFINITY; }
                }
            asm volatile("" ::: "memory");
        }
        float mcs[2], alphas[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            float mx = max32_tree(sv[0][qt], sv[1][qt]);
            {
                auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
                mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
            }
            const float mnew = fmaxf(mrun[qt], mx);
            mcs[qt] = (mnew == -INFINITY) ? 0.f : mnew * c;
            alphas[qt] = __builtin_amdgcn_exp2f(mrun[qt] * c - mcs[qt]);
            mrun[qt] = mnew;
        }
        if (__builtin_amdgcn_ballot_w64(alphas[0] != 1.0f || alphas[1] != 1.0f) != 0) {
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                o[qt][0] = o[qt][0] * alphas[qt];
                o[qt][1] = o[qt][1] * alphas[qt];
            }
        }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const float mc = mcs[qt];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                V8 f;
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = (T)__builtin_amdgcn_exp2f((VAR & 32) ? sv[st >> 1][qt][8 * (st & 1) + e] : fmaf(sv[st >> 1][qt][8 * (st & 1) + e], c, -mc));      // VAR & 32: timing ablation (no fma)
                pf[qt][st] = f;
            }
        }
    };
    // phase boundary: hipcc otherwise hoists the next M phase's PV MFMAs above the barrier into the softmax (register-only instructions are
    // not ordered by s_barrier), which puts matrix work of BOTH groups into the same phase
    auto phase_barrier = [&]() __attribute__((always_inline)) {
        if (!(VAR & 2)) __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        if (!(VAR & 2)) __builtin_amdgcn_sched_barrier(0);
    };
    mphase(0, std::false_type{});
    phase_barrier();
    for (int i = 0; i + 1 < nblk; ++i) {
        vphase(i);
        phase_barrier();
        mphase(i + 1, std::true_type{});
        phase_barrier();
    }
    vphase(nblk - 1);
    phase_barrier();
    if (VAR & 1) __builtin_amdgcn_s_setprio(1);
    if constexpr (SPLIT) pv_split(); else pv();                     // M(nblk): the last block's PV only (staging is over: nblk - 1 + g + 1 >= nblk)
    if (VAR & 1) __builtin_amdgcn_s_setprio(0);
    if (!g) __builtin_amdgcn_s_barrier();                           // pairs with group 1's last phase barrier

    // ---- finalize (as attn32_kernel) ----
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int dd = D & 31;
        const float cand = dd < 8 ? o[qt][1][0] : (dd < 16 ? o[qt][1][4] : o[qt][1][8]);
        const float mine = (h2 == ((dd >> 2) & 1)) ? cand : 0.f;
        auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mine), __float_as_uint(mine), false, false);
        const float l = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
        const float inv = (l > 0.f) ? 1.0f / l : 0.f;
        const int q = q0 + qt * 32 + l31;
        if (q >= p.Nq) continue;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int d = dt * 32 + 8 * rq + 4 * h2;
                if (d < D)
                    *(uint2*)(Op + (long)q * p.ldo + d) = pack4<T>(o[qt][dt][4 * rq] * inv, o[qt][dt][4 * rq + 1] * inv, o[qt][dt][4 * rq + 2] * inv, o[qt][dt][4 * rq + 3] * inv);
            }
    }
}
