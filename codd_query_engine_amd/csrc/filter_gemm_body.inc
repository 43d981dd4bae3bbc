// filter_gemm_body.inc — the statements of gemm_filter_kernel and sqd_filter_kernel (filter_gemm.h includes this file inside both
// function bodies; it is no header of its own).  In scope: MODE, NBQ, EL, RES, SQD and the kernels' parameters.
    static_assert(EL == 0 || (CODD_MFMA16 && kKS == 2), "the int8 mode is written for the 16x16 MFMA geometry");
    static_assert(SQD == 0 || (EL == 1 && RES == 0 && !CODD_BALLOT_HITS && !CODD_BINNED_INLOOP), "the squared-distance form: staged int8 operands, the default hit lists");
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    typedef typename std::conditional<EL == 1, i32x4, acc_t>::type accv_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint4* ldsQ = reinterpret_cast<uint4*>(smem);                        // 2 stages x kQS slices x 32 KiB
    unsigned* lds_w = reinterpret_cast<unsigned*>(smem + kLdsQBytes);    // [0..255] thr / bucket max, [256] hit count
    unsigned* lds_hits = lds_w + kLdsWords;                              // kHitCap x 3 dwords (FILTER only)
    u64* lds_k = reinterpret_cast<u64*>(lds_w);                          // SAMPLE: [0..255] best (score, row) key of the tile per query

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = kQSplit == 1 ? wave : wave % kRowGroups;  // row group of the tile this wave owns
    const int qh = kQSplit == 1 ? 0 : wave / kRowGroups;     // which share of the query blocks
    const int c = lane & (kMB - 1);    // query inside an MFMA query block
    const int qoff = qh * b_piece(NBQ * kQBper32 / kQSplit, 0) * 64;  // first LDS piece of this wave's query blocks
    const int qbase = qh * (NBQ * kQBper32 / kQSplit) * kMB + c;     // this lane's query in query block 0 of the wave

    const int64_t G = gridDim.x;
#if CODD_BLOCKED_TILES
    const int64_t per_wg = (ntiles_run + G - 1) / G;
    const int64_t first_u = (int64_t)blockIdx.x * per_wg, step_u = 1;
    const int64_t my_tiles = first_u >= ntiles_run ? 0 : (first_u + per_wg <= ntiles_run ? per_wg : ntiles_run - first_u);
#else
    const int64_t first_u = blockIdx.x, step_u = G;
    const int64_t my_tiles = ntiles_run > (int64_t)blockIdx.x ? (ntiles_run - blockIdx.x + G - 1) / G : 0;
#endif
    const int T = (int)(my_tiles * nsteps);  // K-steps of this workgroup (< 2^30: rows < 2^32, nsteps <= 64)
    if (T == 0) return;

    if (MODE == MODE_FILTER) {
        if constexpr (SQD == 1) {
            // per query: thr + |q|^2 (a threshold of -inf stays -inf whatever the norm is) and, in the words behind the counter, 2 * scale
            if (tid < 256) {
                const float t = thr[tid];
                lds_w[tid] = __float_as_uint(t == -INFINITY ? t : t + qn2[tid]);
                lds_w[320 + tid] = __float_as_uint(2.0f * qscale[tid]);
            }
        } else {
        // int8: the test runs on acc * rscale[row], so the threshold carries the query's scale (a zero query has
        // scale 0: every score is 0 and its threshold becomes -inf or +inf by sign)
        if (tid < 256) lds_w[tid] = __float_as_uint(EL ? thr[tid] / qscale[tid] : thr[tid]);
        }
        if (tid == 0) lds_w[256] = 0u;
    } else if (MODE == MODE_SAMPLE) {
        if (tid < 256) lds_k[tid] = 0ull;
    }

    constexpr int kSP = NBQ * 256;  // 16-byte pieces of a query slice that are actually staged
    constexpr int kQPn = kSP / kFilterThreads > 0 ? kSP / kFilterThreads : 1;
    constexpr int NQBall = NBQ * kQBper32;       // MFMA query blocks of the pass
    constexpr int NQB = NQBall / kQSplit;        // ... of this wave
    static_assert(NQBall % kQSplit == 0, "query blocks must split evenly");
    accv_t acc[kRS][NQB];
#pragma unroll
    for (int rs = 0; rs < kRS; ++rs)
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
            for (int i = 0; i < kAccRegs; ++i) acc[rs][qb][i] = 0;

    // load cursor (runs kPrefetch steps ahead of the compute cursor)
    int64_t l_u = first_u;  // run-tile ordinal
    int l_s = 0;
    // always issues its 4 loads (a conditional load would make hipcc's vmcnt bookkeeping assume the
    // worst at every join): past the last step the cursor simply stays on the last valid slice
    int l_left = T;
    auto load_a = [&](uint4(&dst)[kRB][4]) {
#pragma unroll
        for (int rb = 0; rb < kRB; ++rb) {
            const int64_t block = (CODD_EXP_SAME_TILE ? 0 : l_u * tile_stride * 8) + wr * kRB + rb;
            const uint4* p = shadow + ((block * nsteps + l_s) * 4) * 64 + lane;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
#if CODD_NT_LOADS
                typedef unsigned v4u __attribute__((ext_vector_type(4)));
                const v4u t = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p + kk * 64));
                dst[rb][kk] = make_uint4(t.x, t.y, t.z, t.w);
#else
                dst[rb][kk] = p[kk * 64];
#endif
            }
        }
        if (--l_left > 0) {
            if (++l_s == nsteps) { l_s = 0; l_u += step_u; }
        }
    };

    uint4 ring[kRing][kRB][4];
#pragma unroll
    for (int i = 0; i < kPrefetch; ++i) load_a(ring[i]);

    // The query operand is a cyclic stream of 64-wide K slices (slice of step t = t mod nsteps),
    // consumed through LDS stages of kQS slices: stage g holds the slices of steps [g*kQS, (g+1)*kQS).
    // Stage 0 is filled here; during step t each thread fetches its part of the slice of step t+kQS
    // and writes it into the other stage after its MFMAs; one barrier per STAGE, not per step.
    int q_s = 0;  // slice that the next staging load fetches
    // every thread stages (loads are unconditional, see load_a); when the slice has fewer pieces than
    // threads, two threads copy the same piece to the same place
    const int stid = kSP >= kFilterThreads ? tid : tid % kSP;
    typedef unsigned q4u __attribute__((ext_vector_type(4)));  // (native vectors: uint4 staging buffers end up as scratch allocas)
#pragma unroll
    for (int sub = 0; sub < (RES ? 2 * kQS : kQS); ++sub) {
        if (RES == 1 && sub >= nsteps) break;  // resident: slice s lives in LDS slice s for the whole kernel
        const uint4* src = qfrag + (int64_t)q_s * kStagePieces + stid;
        uint4* dst = ldsQ + sub * kStagePieces + stid;
        q4u tmp[kQPn];
#pragma unroll
        for (int j = 0; j < kQPn; ++j) tmp[j] = reinterpret_cast<const q4u*>(src)[j * kFilterThreads];
#pragma unroll
        for (int j = 0; j < kQPn; ++j) reinterpret_cast<q4u*>(dst)[j * kFilterThreads] = tmp[j];
        q_s = q_s + 1 == nsteps ? 0 : q_s + 1;
    }
    q4u qreg0[kQPn], qreg1[kQPn];
    if (kQD == 2) {  // the slice step 0 will write to LDS is already on its way
        const uint4* src = qfrag + (int64_t)q_s * kStagePieces + stid;
#pragma unroll
        for (int j = 0; j < kQPn; ++j) qreg1[j] = reinterpret_cast<const q4u*>(src)[j * kFilterThreads];
        q_s = q_s + 1 == nsteps ? 0 : q_s + 1;
    }
    __syncthreads();

#if CODD_STATIC_PRIO
    // the two waves of a SIMD otherwise run in lockstep (same barriers, age-based arbitration) and do
    // their non-MFMA work at the same time; a standing priority makes one of them take the matrix pipe
    // for its whole cluster while the other loads/stages, which staggers them by half a step
    if (__builtin_amdgcn_readfirstlane(tid) >= kFilterThreads / 2) __builtin_amdgcn_s_setprio(CODD_STATIC_PRIO);
#endif
    // ------------------------------------------------------------------------------------------------------------
    // Main loop.  An *interval* is the time between two workgroup barriers and covers one 64-wide K-step of work per
    // wave.  Query staging (loads of slice t+kQS at the top, LDS writes at the bottom) is tied to the interval for
    // every wave.  With CODD_STAGGER the second-dispatched half of the workgroup (waves 4..7 = the SIMD partners of
    // waves 0..3) runs its MFMA work half a K-step late: in interval t it multiplies the second K-half of step t-1,
    // then the first K-half of step t, and issues its corpus loads between the two.  The two waves of a SIMD then reach
    // their loads, waits and epilogues at different times instead of in lockstep (MI355X_MICROARCH.md, "two waves per
    // SIMD", item 9).  Slice hazards with 4 LDS slices: interval t reads slices t-1 and t and writes slice t+2.
    // ------------------------------------------------------------------------------------------------------------
    constexpr int kLag = (CODD_STAGGER && MODE == MODE_FILTER && kKS == 2 && !RES) ? 1 : 0;
    constexpr bool kNoStage = CODD_EXP_NO_QSTAGE || RES == 1;
    // RES = 2 (launched only for rows of exactly 6 K-steps: 768 int8 elements): slices 0 and 1 stay in LDS slices 0 and 1,
    // slices 2..5 alternate between LDS slices 2 and 3.  The unrolled body is one whole tile (6 steps), so which step
    // stages what is known at compile time (a runtime choice would make hipcc drain the corpus prefetch at every join):
    //   step 3 stages slice 4 -> LDS slice 2, step 4: 5 -> 3, step 5: 2 (of the next tile) -> 2, step 0: 3 -> 3,
    //   steps 1 and 2 stage nothing; barriers behind steps 2, 3, 4 and 5.  4 staged slices per tile instead of 6.
    constexpr int kBody = RES == 2 ? 6 : kUnroll;
    static_assert(RES != 2 || (kRing == 3 && kQD == 1 && kQS == 2), "the 6-step body assumes the default ring and stages");
    constexpr bool kBarrierEveryStep = kLag == 1;
    constexpr int kNqbRun = (CODD_EXP_NB < NBQ ? CODD_EXP_NB : NBQ) * kQBper32 / kQSplit;
    const int TI = T + kLag;  // intervals

    // MFMAs of K-halves [KS0, KS1) of the step whose corpus fragments sit in ring slot SLOT and whose query slice is at qs
    auto mfma_part = [&](auto SLOT, auto KS0, auto KS1, const uint4* qs) __attribute__((always_inline)) {
        constexpr int slot = decltype(SLOT)::value;
#pragma unroll
        for (int ks = decltype(KS0)::value; ks < decltype(KS1)::value; ++ks) {
#pragma unroll
            for (int qb = 0; qb < kNqbRun; ++qb) {
                const bf16x8 b = CODD_EXP_NO_LDSREAD ? __builtin_bit_cast(bf16x8, ring[slot][0][(ks + qb) & 3])
                                                     : __builtin_bit_cast(bf16x8, qs[b_piece(qb, ks) * 64]);
#pragma unroll
                for (int rs = 0; rs < kRS; ++rs) {
                    // row block rs lives in 32-row block rs / (32/kMB), sub-block rs % (32/kMB)
                    const bf16x8 a = __builtin_bit_cast(bf16x8, ring[slot][rs / kQBper32][a_piece(rs % kQBper32, ks)]);
                    if constexpr (EL == 1) {
#if CODD_MFMA16
                        acc[rs][qb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), acc[rs][qb], 0, 0, 0);
#endif
                    } else {
#if CODD_MFMA16 && CODD_SHADOW_F16
                    acc[rs][qb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[rs][qb], 0, 0, 0);
#elif CODD_MFMA16
                    acc[rs][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[rs][qb], 0, 0, 0);
#elif CODD_SHADOW_F16
                    acc[rs][qb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[rs][qb], 0, 0, 0);
#else
                    acc[rs][qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[rs][qb], 0, 0, 0);
#endif
                    }
                }
            }
        }
    };
    // threshold test / bucket maxima / dump of the finished tile cu (run-tile ordinal), then clear the accumulators
    auto tile_epilogue = [&](int64_t cu) __attribute__((always_inline)) {
        if (!CODD_NO_EPILOGUE) {
            const int64_t tile = cu * tile_stride;
            const bool ragged = (tile + 1) * kTileRows > n;
#pragma unroll
            for (int rs = 0; rs < kRS; ++rs) {
                const int64_t row0 = tile * kTileRows + wr * (32 * kRB) + rs * kMB;  // + acc_row(r, lane)
                float rsc[kAccRegs];  // int8: this lane's row scales
#pragma unroll
                for (int r = 0; r < kAccRegs; ++r) rsc[r] = (EL && row0 + acc_row(r, lane) < n) ? rscale[row0 + acc_row(r, lane)] : 0.0f;
                // squared-distance form: this lane's row norms — in the filter pass only the smallest of them, for a pre-test that
                // costs one register (a hit's own norm is read again where it is needed: with all four kept, NBQ = 8 spills)
                float rn2[kAccRegs], rnmin = INFINITY;
                if constexpr (SQD == 1) {
#pragma unroll
                    for (int r = 0; r < kAccRegs; ++r) {
                        const bool have = row0 + acc_row(r, lane) < n;
                        const float t = have ? rnorm2[row0 + acc_row(r, lane)] : 0.0f;
                        if (MODE == MODE_FILTER) rnmin = fminf(rnmin, have ? t : INFINITY);
                        else rn2[r] = t;
                    }
                }
                if (MODE == MODE_FILTER) {
#pragma unroll
                    for (int qb = 0; qb < NQB; ++qb) {
                        const float th = CODD_EXP_NO_HITS ? INFINITY : __uint_as_float(lds_w[qbase + qb * kMB]);
                        float v4[kAccRegs];
                        bool some;
                        float s2 = 0.0f;
                        if constexpr (SQD == 1) {
                            // no value of this lane's four rows exceeds fma(max acc * rscale, 2 s_q, -min rnorm2): s_q >= 0, rounding is monotone
                            s2 = __uint_as_float(lds_w[320 + qbase + qb * kMB]);
                            float m = (float)acc[rs][qb][0] * rsc[0];
#pragma unroll
                            for (int r = 1; r < kAccRegs; ++r) m = fmaxf(m, (float)acc[rs][qb][r] * rsc[r]);
                            some = !(__builtin_fmaf(m, s2, -rnmin) < th);
                        } else {
#pragma unroll
                        for (int r = 0; r < kAccRegs; ++r) v4[r] = EL ? (float)acc[rs][qb][r] * rsc[r] : (float)acc[rs][qb][r];
                        float m = v4[0];
#pragma unroll
                        for (int r = 1; r < kAccRegs; ++r) m = fmaxf(m, v4[r]);
                        some = m >= th;
                        }
                        if (__any(some)) {
#if CODD_BALLOT_HITS
                            // one LDS atomic per block that has hits (lane 0 reserves the block's slots, every
                            // hit lane finds its own from the ballots) instead of one contended atomic per register
                            unsigned tot = 0;
#pragma unroll
                            for (int r = 0; r < kAccRegs; ++r)
                                tot += (unsigned)__popcll(__ballot(v4[r] >= th && row0 + acc_row(r, lane) < n));
                            unsigned base = 0;
                            if (lane == 0) base = atomicAdd(&lds_w[256], tot);
                            base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
                            for (int r = 0; r < kAccRegs; ++r) {
                                const bool hit = v4[r] >= th && row0 + acc_row(r, lane) < n;
                                const unsigned long long mk = __ballot(hit);
                                if (hit) {
                                    const unsigned slot = base + __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
                                    if (slot < (unsigned)kHitCap) {
                                        lds_hits[slot * 3 + 0] = __float_as_uint(EL ? v4[r] * qscale[qbase + qb * kMB] : v4[r]);
                                        lds_hits[slot * 3 + 1] = (unsigned)(row0 + acc_row(r, lane));
                                        lds_hits[slot * 3 + 2] = (unsigned)(qbase + qb * kMB);
                                    } else {
                                        atomicOr(&hit_cnt[(qbase + qb * kMB) * kHitCntStride], 0x80000000u);  // see below
                                    }
                                }
                                base += (unsigned)__popcll(mk);
                            }
#else
#pragma unroll
                            for (int r = 0; r < kAccRegs; ++r) {
                                float v = v4[r];
                                const int64_t row = row0 + acc_row(r, lane);
                                if constexpr (SQD == 1) {
                                    unsigned ri = (unsigned)row;      // (rows fit 32 bits; opaque for the reason given below)
                                    asm volatile("" : "+v"(ri));
                                    v = row < n ? __builtin_fmaf((float)acc[rs][qb][r] * rsc[r], s2, -rnorm2[ri]) : -INFINITY;
                                }
                                if ((SQD ? !(v < th) : v >= th) && row < n) {
                                    if constexpr (SQD == 1) {   // the hit's key: v - |q|^2; not a number ranks last
                                        unsigned qi = (unsigned)(qbase + qb * kMB);
                                        asm volatile("" : "+v"(qi));
                                        v -= qn2[qi];
                                        v = v != v ? -INFINITY : v;
                                    }
                                    const unsigned slot = atomicAdd(&lds_w[256], 1u);
                                    if (slot < (unsigned)kHitCap) {
                                        lds_hits[slot * 3 + 0] = __float_as_uint(EL && !SQD ? v * qscale[qbase + qb * kMB] : v);
                                        lds_hits[slot * 3 + 1] = (unsigned)row;
                                        lds_hits[slot * 3 + 2] = (unsigned)(qbase + qb * kMB);
                                    } else {
                                        // workgroup list full (> kHitCap/2 hits inside ONE tile: a dense cluster that many
                                        // queries point at): straight to the query's global list — slow (a returning global
                                        // atomic per hit) but complete, so the query needs no exact-scan fallback.  (Round 1
                                        // poisoned the query's counter here instead and sent it to the fallback: 168 ms per
                                        // batch on a corpus of 64 tight clusters.)
                                        unsigned gq = (unsigned)(qbase + qb * kMB);
                                        asm volatile("" : "+v"(gq));  // (opaque: hipcc otherwise hoists these addresses out of the K loop and spills them)
                                        const unsigned gslot = atomicAdd(&hit_cnt[gq * kHitCntStride], 1u);
                                        if (gslot < (unsigned)cap_q) hits[(int64_t)gq * cap_q + gslot] = make_key(EL && !SQD ? v * qscale[gq] : v, (uint32_t)row);
                                    }
                                }
                            }
#endif
                        }
                    }
                } else if (MODE == MODE_SAMPLE) {
#pragma unroll
                    for (int qb = 0; qb < NQB; ++qb) {
                        u64 best = 0ull;  // this lane's best (score, row) of the block; ties -> lower row, as everywhere
                        float s2 = 0.0f;
                        if constexpr (SQD == 1) s2 = 2.0f * qscale[qbase + qb * kMB];
#pragma unroll
                        for (int r = 0; r < kAccRegs; ++r) {
                            const int64_t row = row0 + acc_row(r, lane);
                            if (!ragged || row < n) {
                                const u64 key = make_key(SQD ? __builtin_fmaf((float)acc[rs][qb][r] * rsc[r], s2, -rn2[r])
                                                             : (EL ? (float)acc[rs][qb][r] * rsc[r] : (float)acc[rs][qb][r]), (uint32_t)row);
                                best = key > best ? key : best;
                            }
                        }
                        atomicMax(reinterpret_cast<unsigned long long*>(&lds_k[qbase + qb * kMB]), (unsigned long long)best);
                    }
                } else {
#pragma unroll
                    for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
                        for (int r = 0; r < kAccRegs; ++r) {
                            const int64_t row = row0 + acc_row(r, lane);
                            if constexpr (SQD == 1) {
                                if (row < n)
                                    dump[(int64_t)(qbase + qb * kMB) * n + row] =
                                        __builtin_fmaf((float)acc[rs][qb][r] * rsc[r], 2.0f * qscale[qbase + qb * kMB], -rn2[r]) - qn2[qbase + qb * kMB];
                            } else
                            if (row < n)
                                dump[(int64_t)(qbase + qb * kMB) * n + row] =
                                    EL ? (float)acc[rs][qb][r] * rsc[r] * qscale[qbase + qb * kMB] : (float)acc[rs][qb][r];
                        }
                }
            }  // rs
        }
#pragma unroll
        for (int rs = 0; rs < kRS; ++rs)
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
                for (int r = 0; r < kAccRegs; ++r) acc[rs][qb][r] = 0;
    };
    auto slice_ptr = [&](int step) -> const uint4* {  // LDS address of the query slice of a step (4 slices, cyclic)
        return ldsQ + ((step + 4) & (2 * kQS - 1)) * kStagePieces + lane + qoff;
    };
    static_assert(kQS == 2 || !kLag, "the staggered schedule is written for 4 LDS slices");

    int64_t c_u = first_u;  // compute cursor: the step a wave finishes in this interval (a lagging wave: step t-1)
    int c_s = 0;
    int64_t w_u = first_u;  // workgroup cursor: the step ALL waves have finished by the end of this interval
    int w_s = 0;
    // TI is walked in whole unrolled bodies: the padding intervals past it recompute the last slice into accumulators
    // nobody reads (`live` gates every side effect), which keeps the loop free of early exits and lets every load stay
    // unconditional
    auto run = [&](auto LAG) __attribute__((always_inline)) {
        constexpr int lag = decltype(LAG)::value;
        for (int t0 = 0; t0 < TI; t0 += kBody) {
            // one interval; IU (position inside the unrolled body) is a compile-time constant, so every register
            // buffer (corpus ring slot, query staging buffer) is chosen by the front end, not by an optimisation pass
            auto k_step = [&](auto IU) __attribute__((always_inline)) {
                constexpr int iu = decltype(IU)::value;
                constexpr int i = iu % kRing;
                const int t = t0 + iu;
                const int stage = t / kQS, sub = t % kQS;
                // RES = 2: iu IS the step inside the tile; what this step stages (slice, LDS slice) or nothing
                constexpr int kStageSlice = iu == 3 ? 4 : (iu == 4 ? 5 : (iu == 5 ? 2 : (iu == 0 ? 3 : -1)));
                constexpr int kStageSlot = iu == 3 ? 2 : (iu == 4 ? 3 : (iu == 5 ? 2 : 3));
                constexpr bool kStagesHere = RES == 2 ? kStageSlice >= 0 : !kNoStage;
                // query slice of step t+kQS: issue now, write to LDS at the end of the interval
                {
                    const uint4* src = qfrag + (int64_t)(RES == 2 ? (kStageSlice < 0 ? 0 : kStageSlice) : q_s) * kStagePieces + stid;
                    if (kStagesHere) {
#pragma unroll
                        for (int j = 0; j < kQPn; ++j) (iu % kQD ? qreg1 : qreg0)[j] = reinterpret_cast<const q4u*>(src)[j * kFilterThreads];
                    }
                    q_s = q_s + 1 == nsteps ? 0 : q_s + 1;
                }
                if constexpr (lag == 0) {
                    const bool live = t < T;
                    // corpus fragments for step t+2 AFTER the query loads: vmcnt retires in order, so the
                    // end-of-step wait for the (L2-served) query slice must not sit behind these HBM loads
                    load_a(ring[(i + kPrefetch) % kRing]);
#if CODD_MFMA_PRIO
                    __builtin_amdgcn_s_setprio(1);
#endif
                    constexpr int kReadSlot6 = iu < 4 ? iu : iu - 2;  // RES = 2: slices 0..5 sit in LDS slices 0,1,2,3,2,3
                    mfma_part(std::integral_constant<int, i>{}, std::integral_constant<int, 0>{}, std::integral_constant<int, kKS>{},
                              RES == 1 ? ldsQ + c_s * kStagePieces + lane + qoff
                                       : (RES == 2 ? ldsQ + kReadSlot6 * kStagePieces + lane + qoff : slice_ptr(t)));
#if CODD_MFMA_PRIO
                    __builtin_amdgcn_s_setprio(0);
#endif
#if CODD_PIN_SCHEDULE && !CODD_EXP_NO_LDSREAD
                    // pin the step's shape: all 8 global loads (4 query, 4 corpus) first so they fly under the
                    // MFMAs; at most a few query fragments live (4 LDS reads up front, then one per MFMA);
                    // the LDS writes of the next query slice last
                    __builtin_amdgcn_sched_group_barrier(0x020, 4 * kRB + (kStagesHere ? kQPn : 0), 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
                    for (int g = 0; g < kKS * kNqbRun - 4; ++g) {
                        __builtin_amdgcn_sched_group_barrier(0x008, kRS, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x008, 4 * kRS, 0);
                    if (kStagesHere) __builtin_amdgcn_sched_group_barrier(0x200, kQPn, 0);
#endif
                    {
                        uint4* dstq = ldsQ + (RES == 2 ? kStageSlot : ((stage + 1) & 1) * kQS + sub) * kStagePieces + stid;
                        if (kStagesHere) {
#pragma unroll
                            for (int j = 0; j < kQPn; ++j)
                                reinterpret_cast<q4u*>(dstq)[j * kFilterThreads] = ((iu + kQD - 1) % kQD ? qreg1 : qreg0)[j];
                        }
                    }
                    if (live && c_s == nsteps - 1) tile_epilogue(c_u);
                    if (++c_s == nsteps) { c_s = 0; c_u += step_u; }
                } else {
                    // ---- lagging wave: second K-half of step t-1, epilogue, corpus loads, first K-half of step t ----
                    const bool live_prev = t >= 1 && t - 1 < T;
                    mfma_part(std::integral_constant<int, (i + kRing - 1) % kRing>{}, std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{},
                              slice_ptr(t - 1));
#if CODD_PIN_SCHEDULE && !CODD_EXP_NO_LDSREAD
                    __builtin_amdgcn_sched_group_barrier(0x020, (kNoStage ? 0 : kQPn), 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
                    for (int g = 0; g < kNqbRun - 4; ++g) {
                        __builtin_amdgcn_sched_group_barrier(0x008, kRS, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x008, 4 * kRS, 0);
#endif
                    if (t >= 1) {
                        if (live_prev && c_s == nsteps - 1) tile_epilogue(c_u);
                        if (++c_s == nsteps) { c_s = 0; c_u += step_u; }
                    } else {
                        // interval 0 multiplied nothing meaningful (there is no step -1): start from clean accumulators
#pragma unroll
                        for (int rs = 0; rs < kRS; ++rs)
#pragma unroll
                            for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
                                for (int r = 0; r < kAccRegs; ++r) acc[rs][qb][r] = 0;
                    }
                    load_a(ring[(i + kPrefetch) % kRing]);  // the slot the second half of step t-1 has just released
                    mfma_part(std::integral_constant<int, i>{}, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, slice_ptr(t));
#if CODD_PIN_SCHEDULE && !CODD_EXP_NO_LDSREAD
                    __builtin_amdgcn_sched_group_barrier(0x020, 4 * kRB, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
                    for (int g = 0; g < kNqbRun - 4; ++g) {
                        __builtin_amdgcn_sched_group_barrier(0x008, kRS, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x008, 4 * kRS, 0);
                    if (!kNoStage) __builtin_amdgcn_sched_group_barrier(0x200, kQPn, 0);
#endif
                    {
                        uint4* dstq = ldsQ + (((stage + 1) & 1) * kQS + sub) * kStagePieces + stid;
                        if (!kNoStage) {
#pragma unroll
                            for (int j = 0; j < kQPn; ++j)
                                reinterpret_cast<q4u*>(dstq)[j * kFilterThreads] = ((iu + kQD - 1) % kQD ? qreg1 : qreg0)[j];
                        }
                    }
                }

                // ---- workgroup bookkeeping (identical in both programs: the barriers must pair up) ----
                // the step every wave has finished by the end of this interval is t - kLag
                const bool wg_tile_end = t >= kLag && t - kLag < T && w_s == nsteps - 1;
                // stage boundary: the other stage is complete and this one is free to be overwritten.
                // A tile end synchronises too (its bookkeeping below needs every wave's epilogue done).
                if (kBarrierEveryStep || (sub == kQS - 1 && !CODD_EXP_NO_BARRIER && !RES) || (RES == 2 && iu >= 2) || wg_tile_end) __syncthreads();
                if (MODE == MODE_FILTER && wg_tile_end) {
                    // empty the workgroup's hit list once it is half full
                    const unsigned cnt = lds_w[256];
                    __syncthreads();  // everyone has read cnt before the next epilogue can move it
                    if (cnt > (unsigned)(CODD_FLUSH_AT)) {
#if CODD_BINNED_INLOOP
                        // (scratch: the 256 free words behind the thresholds and the counter)
                        flush_hits_binned(lds_hits, cnt < (unsigned)kHitCap ? cnt : (unsigned)kHitCap, tid, lds_w + 320, hits, hit_cnt, cap_q);
#else
                        flush_hits(lds_hits, cnt < (unsigned)kHitCap ? cnt : (unsigned)kHitCap, tid, hits, hit_cnt, cap_q);
#endif
                        __syncthreads();
                        if (tid == 0) lds_w[256] = 0u;
                        __syncthreads();
                    }
                }
                if (MODE == MODE_SAMPLE && wg_tile_end) {
                    // all 8 waves have folded this tile into lds_w: publish, reset, and fence the reset
                    // against the next tile's fold
                    if (tid < 256) {
                        // [query][bucket]: the threshold kernel reads rows of it.  (int8: the fold ran on acc * rscale; a
                        // scale >= 0 keeps the order, the query's scale is applied here)
                        u64 key = lds_k[tid];
                        if (SQD && key) key = make_key(key_score(key) - qn2[tid], key_row(key));   // (the fold ran on the fma: the query's norm shifts all of its keys alike)
                        else if (EL && key) key = make_key(key_score(key) * qscale[tid], key_row(key));
                        bucket_key[(int64_t)tid * ntiles_run + w_u] = key;
                        lds_k[tid] = 0ull;
                    }
                    __syncthreads();
                }
                if (t >= kLag && ++w_s == nsteps) { w_s = 0; w_u += step_u; }
            };
            static_for<kBody>(k_step);
        }
    };
    if (kLag && __builtin_amdgcn_readfirstlane(wave) >= kFilterWaves / 2) run(std::integral_constant<int, 1>{});
    else run(std::integral_constant<int, 0>{});

    if (MODE == MODE_FILTER) {
        __syncthreads();
        const unsigned cnt = lds_w[256];
        if (cnt > (unsigned)kHitCap && tid == 0) atomicOr(&flags[FLAG_WG_OVERFLOW], 1u);  // statistics only
        __syncthreads();  // everyone has read cnt (lds_w is about to be reused)
        if (CODD_EXP_NO_FLUSH) return;
        if (CODD_BINNED_FLUSH) flush_hits_binned(lds_hits, cnt < (unsigned)kHitCap ? cnt : (unsigned)kHitCap, tid, lds_w, hits, hit_cnt, cap_q);
        else flush_hits(lds_hits, cnt < (unsigned)kHitCap ? cnt : (unsigned)kHitCap, tid, hits, hit_cnt, cap_q);
    }
