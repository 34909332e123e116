// crossloc_hip: the statements of wgrad_split_kernel and wgrad_pair_kernel - csrc/xl_wgrad.h explains the loop and why this is text
// that the two kernels include between their braces rather than a function they call.  No include guard: not a header of
// declarations.  The including kernel has the template parameter NORM, the argument struct `a`, and has defined
// constexpr bool PAIR = xl_dependent<NORM, ...>;   const float *const xScale; const unsigned *const dyAmax (the pair form's, else nullptr).
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    constexpr int NP = PAIR ? 2 : 3;                                  // planes of an operand: {hi, lo} / three bf16 terms
    constexpr int kUnit = NP * 32;                                    // bytes per row and K-step: NP planes x 16 elements
    constexpr int kOperand = 256 * kUnit;                             // one operand of one stage: 24 KB / 16 KB
    constexpr int kStage = 2 * kOperand;                              // dY side (rows = o) then x side (rows = c)
    constexpr unsigned OOB = 0x80000000u;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;                          // 2 x 4 waves of 128 (o) x 64 (c)

    // block -> (z, o-tile, c-tile, split); the splits of a tile are neighbours (their operand columns share cache lines)
    int b = blockIdx.x;
    const int s = b % a.splits; b /= a.splits;
    const int ct = b % a.nbc; b /= a.nbc;
    const int ot = b % a.nbo;
    const int z = b / a.nbo;
    const int o0 = ot * 256, c0 = ct * 256;
    const int mBeg = s * a.mPerSplit;
    int mEnd = mBeg + a.mPerSplit; if (mEnd > a.M) mEnd = a.M;
    const int nk = mEnd > mBeg ? (mEnd - mBeg + 15) >> 4 : 0;

    const __amdgpu_buffer_rsrc_t srdY = __builtin_amdgcn_make_buffer_rsrc((void *)(a.dy + z * a.zY), 0, (int)a.dyBytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t srdX = __builtin_amdgcn_make_buffer_rsrc((void *)(a.x + z * a.zX), 0, (int)a.xBytes, 0x00020000);
    const int row = tid & 255, th = tid >> 8;                         // my channel of both tiles; my half of the 16 t of a step
    const bool okO = o0 + row < a.Cout, okC = c0 + row < a.Cin;
    float sX = 1.f, sY = 1.f, invAll = 1.f;                            // PAIR: the scales of X and dY, and the inverse of their product
    if constexpr (PAIR) {
        sX = xScale[0];
        invAll = xScale[1];
        const unsigned bits = dyAmax[0];
        int e = 0;
        if (bits >> 23) e = 14 - ((int)(bits >> 23) - 127);            // max |dY| 2^e in [2^14, 2^15)
        e = e > 120 ? 120 : (e < -120 ? -120 : e);
        sY = __builtin_bit_cast(float, (unsigned)(e + 127) << 23);
        invAll *= __builtin_bit_cast(float, (unsigned)(127 - e) << 23);
    }
    float ra[8], rb[8];
    float nSc = 1.f, nSh = 0.f;                                        // NORM: {scale, shift} of (image of the loaded step, my channel)
    int nImg = -1, nLive = 0;                                          // ... that image; how many of my 8 t are inside the split
    auto load_regs = [&](int kk) {                                    // K-step kk -> registers
        const int t0 = mBeg + 16 * kk + 8 * th;
        if constexpr (NORM) {
            nLive = mEnd - t0; nLive = nLive < 0 ? 0 : (nLive > 8 ? 8 : nLive);
            const int n = t0 / a.HW;
            if (okC && nLive > 0 && n != nImg) {
                nImg = n;
                const f32x2 c2 = *reinterpret_cast<const f32x2 *>(a.coef + ((long long)n * a.Cin + c0 + row) * 2);
                if constexpr (PAIR) { nSc = c2[0] * sX; nSh = c2[1] * sX; }   // (fmaf(x, scale s, shift s) = s fmaf(x, scale, shift) to the bit)
                else { nSc = c2[0]; nSh = c2[1]; }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int t = t0 + e;
            const bool live = t < mEnd;
            const unsigned va = (live && okO) ? (unsigned)(((long long)t * a.ldY + o0 + row) * 4) : OOB;
            const unsigned vb = (live && okC) ? (unsigned)(((long long)t * a.ldX + c0 + row) * 4) : OOB;
            ra[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srdY, (int)va, 0, 0));
            rb[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srdX, (int)vb, 0, 0));
        }
    };
    unsigned wOff[NP];                                                // my 16-byte slot of plane p in a row: s ^ swz(row) / rotated rows
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if constexpr (PAIR) wOff[p] = (unsigned)(row * kUnit + (((2 * p + th) ^ swz(row)) * 16));
        else {
            int ph = 2 * p + th + ((row >> 3) & 1);
            if (ph >= 6) ph -= 6;
            wOff[p] = (unsigned)(row * kUnit + ph * 16);
        }
    }
    auto convert = [&](int stage) {                                   // registers -> stage (both operands)
        unsigned char *sb = dsm + stage * kStage;
        unsigned w[NP][4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            if constexpr (PAIR) {                                      // dY: {hi, lo} of dY sY (the tight, data-derived scale)
                const f32x2 v = f32x2{ ra[2 * h], ra[2 * h + 1] } * sY;
                f16x2 vh, vl;
                xl_f16_pair_pk(v, vh, vl);
                w[0][h] = __builtin_bit_cast(unsigned, vh);
                w[1][h] = __builtin_bit_cast(unsigned, vl);
            } else xl_bf16_split3_pk(ra[2 * h], ra[2 * h + 1], w[0][h], w[1][h], w[2][h]);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x4 *>(sb + wOff[p]) = u32x4{ w[p][0], w[p][1], w[p][2], w[p][3] };
        if constexpr (NORM) {                                          // one fmaf, one max: the arithmetic of every apply site (PAIR: times sX)
#pragma unroll
            for (int e = 0; e < 8; ++e) rb[e] = (okC && e < nLive) ? fmaxf(fmaf(rb[e], nSc, nSh), a.normLo) : 0.f;
        }
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            if constexpr (PAIR) {                                      // X: {hi, lo' = (x - hi) 2^11} of x sX (the plan's scale)
                const f32x2 v = NORM ? f32x2{ rb[2 * h], rb[2 * h + 1] } : f32x2{ rb[2 * h], rb[2 * h + 1] } * sX;
                f16x2 vh, vl;
                xl_f16_pair_scaled_pk(v, vh, vl);
                w[0][h] = __builtin_bit_cast(unsigned, vh);
                w[1][h] = __builtin_bit_cast(unsigned, vl);
            } else xl_bf16_split3_pk(rb[2 * h], rb[2 * h + 1], w[0][h], w[1][h], w[2][h]);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x4 *>(sb + kOperand + wOff[p]) = u32x4{ w[p][0], w[p][1], w[p][2], w[p][3] };
    };

    using Frag = std::conditional_t<PAIR, f16x8, bf16x8>;
    const int fr = lane & 31, kh = lane >> 5;
    unsigned slotOff[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if constexpr (PAIR) slotOff[p] = (unsigned)(((2 * p + kh) ^ swz(fr)) * 16);
        else {
            int ph = 2 * p + kh + ((fr >> 3) & 1);
            if (ph >= 6) ph -= 6;
            slotOff[p] = (unsigned)(ph * 16);
        }
    }
    const unsigned frA = (unsigned)((wm * 128 + fr) * kUnit), frB = (unsigned)(kOperand + (wn * 64 + fr) * kUnit);
    Frag fa[NP][4], fas[4], fb[NP][2];                                // dY side (PAIR: {hi, lo} + hs); X side (PAIR: {hi, lo'})
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    auto ldA = [&](int stage, int p, int i) { return *reinterpret_cast<const Frag *>(dsm + stage * kStage + frA + i * 32 * kUnit + slotOff[p]); };
    auto ldB = [&](int stage, int p, int j) { return *reinterpret_cast<const Frag *>(dsm + stage * kStage + frB + j * 32 * kUnit + slotOff[p]); };
    auto mma = [&](const Frag (&x)[2], const Frag (&d)[4]) {          // one term: X side x dY side
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if constexpr (PAIR) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[j], d[i], acc[i][j], 0, 0, 0);
                else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[j], d[i], acc[i][j], 0, 0, 0);
            }
    };

    // (the end of a K-step - the loads of step kk + 2, the wait, the barrier - is the same text in both forms' steps: as one
    //  lambda that both call it changed the register assignment of the NORM kernels)
    if (nk > 0) {
        load_regs(0);
        convert(0);
        if (nk > 1) load_regs(1);
        __syncthreads();
        for (int kk = 0; kk < nk; ++kk) {
            const int st = kk & 1;
            if constexpr (PAIR) {
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[0][i] = ldA(st, 0, i);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[1][j] = ldB(st, 1, j);
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[1][i] = ldA(st, 1, i);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[0][j] = ldB(st, 0, j);
#pragma unroll
                for (int i = 0; i < 4; ++i) fas[i] = xl_f16_hs(fa[0][i]);
                mma(fb[1], fas);                                           // lo'(X) x hs(dY)
                __builtin_amdgcn_sched_barrier(0);
                // lo(dY) x hi(X) with the conversion of step kk + 1 threaded through it (the other stage: every wave finished
                // reading it before the barrier that ended step kk - 1)
                mma(fb[0], fa[1]);
                if (kk + 1 < nk) convert(st ^ 1);
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 10, 0);
                    if (g == 3 || g == 7) __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 2 < nk) load_regs(kk + 2);                        // (the registers are free again)
                // my LDS writes are done, every wave has read this step's stage - but NOT vmcnt(0) (see the six-pass step below)
                __builtin_amdgcn_s_waitcnt(0x0070 | 0xC00F);               // lgkmcnt(0)
                __builtin_amdgcn_sched_barrier(0);                         // (nothing of the next step may move above the barrier, nothing of
                __builtin_amdgcn_s_barrier();                              //  this one below it: the bare s_barrier carries no fence - ADVICE r4)
                __builtin_amdgcn_sched_barrier(0);
                mma(fb[0], fa[0]);                                         // hi x hi
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[2][j] = ldB(st, 2, j);
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[0][i] = ldA(st, 0, i);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[1][j] = ldB(st, 1, j);
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[1][i] = ldA(st, 1, i);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[0][j] = ldB(st, 0, j);
                mma(fb[2], fa[0]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[2][i] = ldA(st, 2, i);
                mma(fb[1], fa[1]);
                __builtin_amdgcn_sched_barrier(0);
                mma(fb[0], fa[2]);
                __builtin_amdgcn_sched_barrier(0);
                // terms 4 and 5 with the conversion of step kk + 1 threaded through them (the other stage: every wave finished
                // reading it before the barrier that ended step kk - 1)
                mma(fb[1], fa[0]);
                if (kk + 1 < nk) convert(st ^ 1);
                mma(fb[0], fa[1]);
#pragma unroll
                for (int g = 0; g < 12; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
                    if (g == 5 || g == 11) __builtin_amdgcn_sched_group_barrier(0x200, 3, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 2 < nk) load_regs(kk + 2);                        // (the registers are free again)
                // my LDS writes are done, every wave has read this step's stage - but NOT vmcnt(0): __syncthreads() would hold
                // all eight waves until the loads just issued are back, a memory latency per K-step with nothing under it;
                // their wait belongs to the conversion one step later (the compiler counts it there)
                __builtin_amdgcn_s_waitcnt(0x0070 | 0xC00F);               // lgkmcnt(0)
                __builtin_amdgcn_sched_barrier(0);                         // (nothing of the next step may move above the barrier, nothing of
                __builtin_amdgcn_s_barrier();                              //  this one below it: the bare s_barrier carries no fence - ADVICE r4)
                __builtin_amdgcn_sched_barrier(0);
                mma(fb[0], fa[0]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- store the partial tile (PAIR: un-scaled, exact): row o = lane & 31 (+ 32 i), 4 consecutive c per quad
    float *P = a.partial + ((long long)z * a.splits + s) * (long long)a.Cout * a.Cin;
    const int rhalf = kh * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int o = o0 + wm * 128 + i * 32 + fr;
        if (o >= a.Cout) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + wn * 64 + j * 32 + rhalf + 8 * q;
                if (c < a.Cin) {
                    const f32x4 v = f32x4{ acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3] };
                    if constexpr (PAIR) *reinterpret_cast<f32x4 *>(P + (long long)o * a.Cin + c) = v * invAll;
                    else *reinterpret_cast<f32x4 *>(P + (long long)o * a.Cin + c) = v;
                }
            }
    }
