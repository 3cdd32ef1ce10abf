// attention32.inc -- CLIP self-attention (head_dim 64, 321..608 keys) as ONE wave per SIMD on 32x32x16 MFMAs.
// Included by attention_diag.inc, i.e. by attention.hip in the diagnostic build only (shares AttnArgs and the inline-asm LDS helpers).
//
// attn64r (above) runs two 3-sub-block waves per SIMD and leaves the overlap of the matrix pipe with the softmax VALU
// stream to the hardware's wave arbitration; rocprofv3 shows it MFMA-busy 17 % of the time with the waves parked or
// stalled at issue for the rest (DESIGN.md section 6).  This kernel follows the other school (MI355X_MICROARCH.md, "one
// wave per SIMD, 512-register kernel"): 4 waves per workgroup, each with the whole 512-register budget, each owning up to
// FIVE 32-query blocks, and the overlap is written into the instruction stream.
//
//   S^T[kv,q] = K Q^T      A = 32 K rows from LDS (ds_read_b128, 16-B-chunk XOR swizzle), B = Q in VGPRs (16 d per MFMA)
//   O^T[d,q]  = V^T P^T    A = V^T via ds_read_b64_tr_b16, B = P^T
// 32x32 C/D layout: col = lane & 31 (one query per lane pair), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  A lane's 16
// score registers, exponentiated and packed in register order, ARE the two B operands of the PV MFMAs (k-slot 8 h + e of
// kv step j <-> register 8 j + e); the V transpose reads are addressed to match.  P never touches LDS.
//
// What bounds it: per (32-query block, 32-key step) there are 11 MFMAs (4 QK + 1 reference + 4 PV + 2 row sums) = 352 cycles
// of the SIMD's matrix pipe, and 16 v_exp_f32 (11 cycles each alone) + 8 packs + 8 v_max3 = ~240 cycles of its VALU.  A
// hand-placed stream of exactly this mix runs at 364 cycles per 11 MFMAs (tools/attn32_slot_probe.hip): the two pipes overlap
// almost completely IF the wave never waits -- so the main loop is one software pipeline over the flattened (step, block)
// sequence: iteration i issues the MFMAs of QK(i+1) and PV(i-1) around the softmax of block i, across step boundaries.
//
// The running maximum is lazy and SPECULATIVE: scores are produced relative to a per-query reference m_ref (it enters through
// the MFMA itself: a fifth k-step whose A operand is a constant 1 in slot 0 and whose B operand carries -m_ref, kept
// bf16-representable), the exps are issued against it from the first gap of the iteration on, the maximum is built beside
// them, and only the last instruction tests whether a score exceeded the reference by more than 8 (log2 units).  In that rare
// case (and in step 0, which has no reference yet) the block's P is recomputed against the new reference and the block's
// accumulators are rescaled -- the score tile is intact until QK(i+2).  Row sums come from an all-ones A operand.
//
// Accumulators (5 blocks x (2 O^T tiles + 1 sum tile) x 16 registers = 240) live in AGPRs, score tiles in VGPRs; all MFMAs
// and all softmax instructions of the main loop are volatile asm in issue order (hipcc neither orders pure VALU code against
// asm MFMAs nor keeps accumulators out of the VGPR file by itself).  K/V panel staging: LDS-DMA in 64-row granules, one
// barrier for the first granule and one for the rest (the panel has landed long before step 2 is reached).

#include "slots32.h"

#define A32_VR_ALL "v"(vr[0][0][0]), "v"(vr[0][0][1]), "v"(vr[0][1][0]), "v"(vr[0][1][1]), "v"(vr[1][0][0]), "v"(vr[1][0][1]), \
                   "v"(vr[1][1][0]), "v"(vr[1][1][1])
#define A32_KF_ALL "v"(kf[0]), "v"(kf[1]), "v"(kf[2]), "v"(kf[3])
template <typename T, int NB, bool DBG>
__device__ __forceinline__ void attn32_body(const AttnArgs& a, char* smem, const int b, const int h, const int blk0) {
    constexpr int RB = 128, KC = 608, NG = 10, NBX = NB > 0 ? NB : 1;
    constexpr float RESCALE_TH = 8.0f;
    char* Klds = smem;
    char* Vlds = smem + KC * RB;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q31 = lane & 31, hh = lane >> 5;
    // diagnostic stamps (DBG instantiation only: even a never-taken `if (a.dbg)` is a scalar branch per step): 32 s_memtime
    // slots per wave; a.abl != 0: no per-step stamps (each costs ~100 cycles)
    unsigned long long* dbgp = nullptr;
    if constexpr (DBG) dbgp = a.dbg + (((size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 4 + wave) * 32;
    auto stamp = [&](int slot) {
        if constexpr (DBG) {
            if (a.abl == 0 || slot < 4 || slot >= 30) {
                const unsigned long long t = __builtin_amdgcn_s_memtime();
                if (lane == 0) dbgp[slot] = t;
            }
        }
    };
    stamp(0);

    // ---- Q: B operand of QK, lane (q, hh) holds d = 16 j + 8 hh .. + 7 of its query row for the four d-steps j ----
    // The loads are asm so that hipcc does not count them: beside LDS-DMA it would wait vmcnt(0) -- the whole panel -- in front of
    // their first use, every step.  They are issued first and waited for (vmcnt(40) = everything but this wave's 40 DMAs)
    // in front of the main loop, so their latency passes under the DMA issue.
    u32x4 qf[NBX][4];
    if constexpr (NB > 0) {
        const char* qbase = a.q + ((size_t)b * a.q_bs + (size_t)h * 64) * 2;
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            const int qr = min((blk0 + s) * 32 + q31, a.n_q - 1);
            const char* qp = qbase + ((size_t)qr * a.q_rs + 8 * hh) * 2;
            asm volatile("global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %4, off offset:32\n\t"
                         "global_load_dwordx4 %2, %4, off offset:64\n\tglobal_load_dwordx4 %3, %4, off offset:96"
                         : "=&v"(qf[s][0]), "=&v"(qf[s][1]), "=&v"(qf[s][2]), "=&v"(qf[s][3]) : "v"(qp) : "memory");
        }
    }

    // ---- K/V panel: 10 granules of 64 rows = 8 pieces of 8 rows; wave w moves pieces 8 gi + w and 8 gi + 4 + w of K and V ----
    // SGPR-base form: the per-lane byte offset inside a piece (row lrow, swizzled chunk) is computed once, the piece's base is
    // scalar arithmetic -- no VALU address math per DMA (the builtin spends ~15 VALU instructions on each).  Pieces that reach
    // past n_kv (clamped copies of the last row, masked in the last step) take per-lane offsets from the panel base.
    // (The builtin spends ~15 VALU instructions of address arithmetic per DMA; the SGPR-base asm form of the GEMMs was measured
    // here and is SLOWER -- 8.2k vs 7.1k cycles to issue the panel: the issue is paced by the ~23 B/cycle/CU the DMAs move.)
    {
        const char* kbase = a.k + ((size_t)b * a.k_bs + (size_t)h * 64) * 2;
        const char* vbase = a.v + ((size_t)b * a.v_bs + (size_t)h * 64) * 2;
        const int lrow = lane >> 3, cpos = lane & 7;
#pragma unroll
        for (int gi = 0; gi < NG; ++gi)
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                int piece = gi * 8 + half * 4 + wave;
                if (piece >= KC / 8) piece -= 4;              // granule 9 has 4 pieces: the second round repeats them (same bytes,
                                                              // same place) so that every wave issues exactly 4 DMAs per granule
                const int row = piece * 8 + lrow;
                const int kchunk = cpos ^ ((row >> 1) & 7);   // reader: chunk ^ ((kv >> 1) & 7), conflict-free for 32-row b128 reads
                const int vchunk = cpos ^ (((row >> 1) & 1) << 2);
                const int srow = min(row, a.n_kv - 1);        // rows >= n_kv: clamped copies, masked in the last step
                __builtin_amdgcn_global_load_lds(GLOBAL_PTR(kbase + ((size_t)srow * a.k_rs) * 2 + kchunk * 16),
                                                 LDS_PTR(Klds + piece * 1024), 16, 0, 0);
                __builtin_amdgcn_global_load_lds(GLOBAL_PTR(vbase + ((size_t)srow * a.v_rs) * 2 + vchunk * 16),
                                                 LDS_PTR(Vlds + piece * 1024), 16, 0, 0);
            }
    }
    // The first granule (rows 0..63, steps 0 and 1) has landed for this wave when at most 36 of its 40 DMAs are outstanding; the
    // barrier extends that to every wave's pieces.  Everything else is waited for once, in front of step 2: issuing the panel
    // takes ~7k cycles by itself and two steps ~5k, so there is nothing left to overlap by then, and a barrier every granule
    // costs 500-800 cycles of skew each (measured).
    auto before_step = [&](int st) {                          // called by every wave for st = 0, 1, 2, ... (uniform control flow)
        if (st == 0) asm volatile("s_waitcnt vmcnt(36)" ::: "memory");
        else if (st == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (st == 0 || st == 2) {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_barrier" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    stamp(1);
    const int steps = (a.n_kv + 31) >> 5;
    if constexpr (NB == 0) {
        for (int st = 0; st < steps; ++st) before_step(st);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    } else {
        f32x16 o[NB][2], osum[NB];
        float m_ref[NB];
        u32x4 qx[NB];
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            m_ref[s] = 0.f;
            qx[s] = u32x4{0u, 0u, 0u, 0u};
            asm volatile("" : "+v"(qx[s]));                  // opaque: keep the four registers of each tuple instead of rebuilding
                                                              // {w, 0, 0, 0} with v_movs in front of every reference MFMA
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[s][0][r] = 0.f; o[s][1][r] = 0.f; osum[s][r] = 0.f; }
        }
        const unsigned one2 = T::pack2(1.0f, 1.0f);
        u32x4 ones = {one2, one2, one2, one2};
        u32x4 kx = {hh == 0 ? T::pack2(1.0f, 0.0f) : 0u, 0u, 0u, 0u};            // A operand of the reference k-step
        float th = RESCALE_TH;
        asm volatile("" : "+v"(ones), "+v"(kx), "+v"(th));   // resident VGPRs (otherwise rebuilt from SGPRs in front of each use)
        unsigned kptr[4], vptr[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) kptr[j] = lds_addr(Klds) + q31 * RB + (((2 * j + hh) ^ ((q31 >> 1) & 7)) << 4);
        {
            // transpose read: the 16-lane group G = lane >> 4 serves k-slot half hh = G >> 1 and d-rows 16 (G & 1) .. + 15; inside
            // the group lane i16 = a + 4 bb SUPPLIES row bb, 8-byte piece a, and RECEIVES d-row i16, rows bb' = 0..3
            const int dblk = (lane >> 4) & 1, i16 = lane & 15, pa = i16 & 3, bb = i16 >> 2, flip = (bb >> 1) & 1;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
                vptr[dt] = lds_addr(Vlds) + (4 * hh + bb) * RB + ((dt ^ flip) << 6) + (4 * dblk + pa) * 8;
        }
        // ragged last step: bit r of `dead` = score register r of this lane belongs to a key >= n_kv
        unsigned dead = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) dead |= ((steps - 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh >= a.n_kv ? 1u : 0u) << r;
        const bool ragged = (a.n_kv & 31) != 0;

        u32x4 kf[4];
        u32x2 vr[2][2][2];                                    // V^T fragments [d-tile][kv half j][slot half c]
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int j = 0; j < 2; ++j) { vr[dt][j][0] = u32x2{0u, 0u}; vr[dt][j][1] = u32x2{0u, 0u}; }
        auto k_request = [&]() {
#pragma unroll
            for (int j = 0; j < 4; ++j) { kf[j] = lds_b128_asm<0>(kptr[j]); kptr[j] += 32 * RB; }
        };
        // V^T fragments of one 16-key half of the next step the B stream enters; the pointers advance after the second half
        auto v_request0 = [&]() {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) { vr[dt][0][0] = lds_tr16_asm<0>(vptr[dt]); vr[dt][0][1] = lds_tr16_asm<8 * RB>(vptr[dt]); }
        };
        auto v_request1 = [&]() {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                vr[dt][1][0] = lds_tr16_asm<16 * RB>(vptr[dt]);
                vr[dt][1][1] = lds_tr16_asm<24 * RB>(vptr[dt]);
                vptr[dt] += 32 * RB;
            }
        };

        f32x16 S[2];                                          // score tiles, by the parity of the flattened (step, block) index
        u32x4 pf[2][2];                                       // P^T operands [same parity][kv half j]
#pragma unroll
        for (int p = 0; p < 2; ++p) { pf[p][0] = u32x4{0u, 0u, 0u, 0u}; pf[p][1] = u32x4{0u, 0u, 0u, 0u}; }

        // One step = NB iterations of the pipeline.  PAR = parity of (step * NB): fixes which score / P buffer a block uses.
        // Iteration (st, blk):  A stream = QK of the next block in flattened order ((st, blk+1), or (st+1, 0) from the last
        // iteration: its K fragments are requested at the top of that iteration and the MFMAs start one pair later, the
        // reference MFMA trailing behind the last slot), B stream = PV of the previous block ((st, blk-1), or (st-1, NB-1) in
        // iteration 0; at the very start that is a product of zeros), gaps = softmax of (st, blk).
        auto step = [&](const int st, auto par_tag) {
            constexpr int PAR = decltype(par_tag)::value;
            const bool has_next = st + 1 < steps;
            const bool masked = ragged && !has_next;
#pragma unroll
            for (int blk = 0; blk < NB; ++blk) {
                const int fp = (PAR * NB + blk) & 1;          // folds: blk is an unrolled constant
                const int pb = blk > 0 ? blk - 1 : NB - 1, nb = blk + 1 < NB ? blk + 1 : 0;
                const bool last = blk == NB - 1;
                f32x16& sc = S[fp];
                f32x16& sn = S[fp ^ 1];
                // K fragments of the next step.  NB >= 2: fragment j is re-requested right behind its last use, the MFMA of pair j in
                // iteration NB - 2 (QK of this step's last block), so the last iteration finds them landed.  NB = 1: every iteration
                // multiplies the next step's K; requested at the top, the A stream starts one pair later and its reference MFMA
                // trails behind the last slot.  Past the last step this reads 32 rows beyond the K panel (the head of the V
                // panel); the tile built from them is never used.
                const bool kreq = NB >= 2 && blk == NB - 2;
                // (in the loop, before_step(st + 1) does something for st + 1 == 2 only: one never-taken branch per step)
                if ((kreq || NB == 1) && __builtin_expect(st == 1, 0)) before_step(2);
                if (NB == 1) k_request();
                auto k_rerequest = [&](int j) { if (kreq) { kf[j] = lds_b128_asm<0>(kptr[j]); kptr[j] += 32 * RB; } };
                if (__builtin_expect(masked, 0)) {
                    if (NB == 1) asm volatile("s_nop 7\n\ts_nop 3" : "+v"(sc));     // completed by the MFMA just issued
#pragma unroll
                    for (int r = 0; r < 16; ++r) sc[r] = (dead >> r) & 1 ? -INFINITY : sc[r];
                    asm volatile("" : "+v"(sc));
                }
                float e[16], m0, m1, m2, m3, m4;
                unsigned pk[8];
                unsigned long long runaway = 0;
                // pair i: MFMA A = k-step kk of QK(nb) into sn (ka = 0: none), gap 2 i, MFMA B = MFMA i of PV(pb), gap 2 i + 1
                auto pair = [&](int i, int ka, int kk) {
                    f32x16& sv = sn;
                    const u32x4 ma = kk < 4 ? kf[kk] : kx, mb = kk < 4 ? qf[nb][kk] : qx[nb];
                    const int j = i / 3, w = i % 3;
                    f32x16& av = w == 2 ? osum[pb] : o[pb][w];
                    const u32x4 vfw = {vr[w & 1][j][0][0], vr[w & 1][j][0][1], vr[w & 1][j][1][0], vr[w & 1][j][1][1]};
                    const u32x4 mab = w == 2 ? ones : vfw, mbb = pf[fp ^ 1][j];
                    switch (i) {
                        case 0: if (NB == 1) A32_PAIR(P01N); else A32_PAIR(P01); break;
                        case 1: A32_PAIR(P23); break;
                        case 2: A32_PAIR(P45); break;
                        case 3: A32_PAIR(P67); break;
                        default: A32_PAIR(P89); break;
                    }
                };
                // V^T of the step the B stream is about to enter (requested in iteration 0, see below): first use of half 0 in pair 0,
                // of half 1 in pair 3.  LDS returns in order; behind the half-0 reads there are the 4 half-1 reads and, in a last
                // iteration, the 4 K reads just issued.
                const bool new_v = pb == 0;
                if (NB == 1) {
                    // [V half 0][V half 1][K] in flight, in that order
                    A32_WAIT("lgkmcnt(8)", A32_VR_ALL);
                    // no MFMA A in front of the first exps -- the tile they read was completed by the MFMA issued at the end of the
                    // previous iteration, and only the 4 states of P01N lie in between
                    asm volatile("s_nop 7" : "+v"(sc));
                    pair(0, 0, 0);
                    A32_WAIT("lgkmcnt(0)", A32_KF_ALL, A32_VR_ALL);
                    pair(1, 1, 0);
                    pair(2, 2, 1);
                    v_request0();                             // MFMAs 0..2 of PV(st-1) have read half 0 of the old step
                    pair(3, 2, 2);
                    pair(4, 2, 3);
                } else {
                    // LDS returns in order.  In flight at the top: iteration 1 -- [V half 0][V half 1] (+ for NB = 2 the K fragments
                    // 0..2 in front of half 0 and fragment 3 between the halves); last iteration -- the K fragments.
                    if (new_v && last) A32_WAIT("lgkmcnt(5)", A32_KF_ALL, A32_VR_ALL);          // NB = 2: K 0..2 and V half 0 landed
                    else if (new_v) A32_WAIT("lgkmcnt(4)", A32_VR_ALL);
                    else if (last) A32_WAIT("lgkmcnt(0)", A32_KF_ALL);
                    pair(0, 1, 0); k_rerequest(0);
                    pair(1, 2, 1); k_rerequest(1);
                    pair(2, 2, 2); k_rerequest(2);
                    if (blk == 0) v_request0();               // MFMAs 0..2 of PV(st-1, NB-1) have read half 0 of the old step
                    // V half 1 (first use: MFMA B of pair 3); behind it in the queue: the K fragments just re-requested (NB = 3)
                    if (new_v && kreq) A32_WAIT("lgkmcnt(3)", A32_VR_ALL);
                    else if (new_v) A32_WAIT("lgkmcnt(0)", A32_VR_ALL, A32_KF_ALL);
                    pair(3, 2, 3); k_rerequest(3);
                    pair(4, 2, 4);
                }
                {
                    f32x16& av = osum[pb];
                    const u32x4 mab = ones, mbb = pf[fp ^ 1][1];
                    asm volatile(A32_MFB P10_STR : [accb] "+a"(av), P10_OUT : [mab] "v"(mab), [mbb] "v"(mbb), P10_IN);
                }
                if (blk == 0) v_request1();                   // ... and MFMAs 3..5 half 1 (NB = 1: blk is always 0)
                // a runaway score: new reference, recompute P, rescale the block's accumulators
                if (__builtin_expect(runaway != 0, 0)) {
                    float mx = sc[0];
#pragma unroll
                    for (int r = 1; r < 16; ++r) mx = __builtin_fmaxf(mx, sc[r]);
                    const unsigned u = __float_as_uint(mx);
                    const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
                    float d = __builtin_fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
                    d = d > RESCALE_TH ? d : 0.f;             // only the rows that ran away themselves move: a row's result does not
                                                              // depend on what shares its block (d = 0 reproduces the speculative P)
                    const unsigned mw = T::pack2(-(m_ref[blk] + d), 0.0f);      // the new reference, rounded to 16 bits
                    const float m_new = -T::lo(mw);
                    d = m_new - m_ref[blk];
                    m_ref[blk] = m_new;
                    qx[blk][0] = hh == 0 ? mw : 0u;
                    asm volatile("" : "+v"(qx[blk]));
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        pk[q] = T::pack2(__builtin_amdgcn_exp2f(sc[2 * q] - d), __builtin_amdgcn_exp2f(sc[2 * q + 1] - d));
                    {
                        const float alpha = __builtin_amdgcn_exp2f(-d);
                        // (NB = 1: the B stream of this very iteration accumulated into this block's tiles)
                        asm volatile("s_nop 7\n\ts_nop 7" : "+a"(o[blk][0]), "+a"(o[blk][1]), "+a"(osum[blk]));
#pragma unroll
                        for (int r = 0; r < 16; ++r) { o[blk][0][r] *= alpha; o[blk][1][r] *= alpha; osum[blk][r] *= alpha; }
                        // back into the accumulator file before the paths join (a VGPR-class phi would copy all 48 registers on
                        // the common path too)
                        asm volatile("" : "+a"(o[blk][0]), "+a"(o[blk][1]), "+a"(osum[blk]));
                    }
                }
                pf[fp][0] = u32x4{pk[0], pk[1], pk[2], pk[3]};
                pf[fp][1] = u32x4{pk[4], pk[5], pk[6], pk[7]};
                asm volatile("" : "+v"(pf[fp][0]), "+v"(pf[fp][1]));
                // NB = 1: the reference MFMA of the shifted A stream comes behind the test -- the tile it completes belongs to the
                // block whose reference may just have moved
                if (NB == 1) Mfma32Asm<T>::next(sn, kx, qx[nb]);
            }
            // Loop-carried accumulators must be AGPR values on the back edge: where VGPRs are free (small NB) the allocator
            // otherwise keeps them there and copies 48 registers into the accumulator file and back in every iteration.
#pragma unroll
            for (int s = 0; s < NB; ++s) asm volatile("" : "+a"(o[s][0]), "+a"(o[s][1]), "+a"(osum[s]));
        };

#pragma unroll
        for (int s = 0; s < NB; ++s) A32_WAIT("vmcnt(40)", "v"(qf[s][0]), "v"(qf[s][1]), "v"(qf[s][2]), "v"(qf[s][3]));
        stamp(2);
        before_step(0);
        stamp(3);
        k_request();
        A32_WAIT("lgkmcnt(0)", A32_KF_ALL);
        // Reference pre-pass: the row maxima over the first 32 keys become the initial references, so that step 0 runs the
        // speculative stream like every other step (recomputing P for every block of step 0 cost ~1k cycles per block).
        // Block 0 goes last and keeps its tile: it is the pipeline's first score tile, reference subtracted by hand.
        auto qk4 = [&](int blk) {
            f32x16& t = S[blk & 1];
            Mfma32Asm<T>::first(t, kf[0], qf[blk][0]);
            Mfma32Asm<T>::next(t, kf[1], qf[blk][1]);
            Mfma32Asm<T>::next(t, kf[2], qf[blk][2]);
            Mfma32Asm<T>::next(t, kf[3], qf[blk][3]);
        };
        auto take_reference = [&](int blk) {
            f32x16& t = S[blk & 1];
            float mx = max3f(t[0], t[1], t[2]);
            mx = max3f(mx, t[3], t[4]); mx = max3f(mx, t[5], t[6]); mx = max3f(mx, t[7], t[8]); mx = max3f(mx, t[9], t[10]);
            mx = max3f(mx, t[11], t[12]); mx = max3f(mx, t[13], t[14]); mx = __builtin_fmaxf(mx, t[15]);
            const unsigned u = __float_as_uint(mx);
            const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
            mx = __builtin_fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
            const unsigned mw = T::pack2(-mx, 0.0f);          // rounded to 16 bits: it travels as an MFMA operand
            m_ref[blk] = -T::lo(mw);
            qx[blk][0] = hh == 0 ? mw : 0u;
            asm volatile("" : "+v"(qx[blk]));
        };
        qk4(NB - 1);
#pragma unroll
        for (int blk = NB - 2; blk >= 0; --blk) {
            qk4(blk);                                         // 4 MFMAs = 128 cycles behind the tile read below
            asm volatile("" : "+v"(S[(blk + 1) & 1]));
            take_reference(blk + 1);
        }
        asm volatile("s_nop 7\n\ts_nop 7" : "+v"(S[0]));
        take_reference(0);
#pragma unroll
        for (int r = 0; r < 16; ++r) S[0][r] -= m_ref[0];
        asm volatile("" : "+v"(S[0]));
        using P0 = std::integral_constant<int, 0>;
        using P1 = std::integral_constant<int, 1>;
        int st = 0, fpl;                                      // fpl: buffer parity of the last block
        if constexpr ((NB & 1) != 0) {
            for (; st + 1 < steps; st += 2) { step(st, P0{}); stamp(4 + st); step(st + 1, P1{}); stamp(5 + st); }
            if (st < steps) { step(st, P0{}); stamp(4 + st); fpl = (NB - 1) & 1; }
            else fpl = (NB + NB - 1) & 1;
        } else {
            for (; st < steps; ++st) { step(st, P0{}); stamp(4 + st); }
            fpl = (NB - 1) & 1;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // granules beyond the last step (short n_kv)
        // drain: PV of the last block
        A32_WAIT("lgkmcnt(0)", A32_VR_ALL, A32_KF_ALL);
        {
            const u32x4 v00 = {vr[0][0][0][0], vr[0][0][0][1], vr[0][0][1][0], vr[0][0][1][1]}, v01 = {vr[0][1][0][0], vr[0][1][0][1], vr[0][1][1][0], vr[0][1][1][1]};
            const u32x4 v10 = {vr[1][0][0][0], vr[1][0][0][1], vr[1][0][1][0], vr[1][0][1][1]}, v11 = {vr[1][1][0][0], vr[1][1][0][1], vr[1][1][1][0], vr[1][1][1][1]};
            u32x4 p0 = fpl ? pf[1][0] : pf[0][0], p1 = fpl ? pf[1][1] : pf[0][1];
            asm volatile("s_nop 3" : "+v"(p0), "+v"(p1));
            Mfma32Asm<T>::run(o[NB - 1][0], v00, p0);
            Mfma32Asm<T>::run(o[NB - 1][1], v10, p0);
            Mfma32Asm<T>::run(osum[NB - 1], ones, p0);
            Mfma32Asm<T>::run(o[NB - 1][0], v01, p1);
            Mfma32Asm<T>::run(o[NB - 1][1], v11, p1);
            Mfma32Asm<T>::run(osum[NB - 1], ones, p1);
        }

        // asm MFMAs: pad their write-back latency by hand, then tie every accumulator to a statement behind the padding
        asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
#pragma unroll
        for (int s = 0; s < NB; ++s) { asm volatile("" : "+a"(o[s][0])); asm volatile("" : "+a"(o[s][1])); asm volatile("" : "+a"(osum[s])); }

        stamp(30);
        // lane (q, hh) holds d = 32 dt + 8 c + 4 hh + 0..3 (c = r >> 2): a half swap between the lane pair turns that into 8
        // consecutive d per lane (hh = 0: c even, hh = 1: c odd) -> 16-byte stores
        char* obase = a.o + ((size_t)b * a.o_bs + (size_t)h * 64) * 2;
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            const float inv = 1.0f / osum[s][0];
            const int qr = (blk0 + s) * 32 + q31;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int cp = 0; cp < 2; ++cp) {
                    const int ce = 2 * cp, co = 2 * cp + 1;
                    unsigned e0 = T::pack2(o[s][dt][4 * ce] * inv, o[s][dt][4 * ce + 1] * inv);
                    unsigned e1 = T::pack2(o[s][dt][4 * ce + 2] * inv, o[s][dt][4 * ce + 3] * inv);
                    unsigned o0 = T::pack2(o[s][dt][4 * co] * inv, o[s][dt][4 * co + 1] * inv);
                    unsigned o1 = T::pack2(o[s][dt][4 * co + 2] * inv, o[s][dt][4 * co + 3] * inv);
                    // swap(A = even, B = odd): A.upper <-> B.lower; afterwards hh = 0 holds (own even, partner's even),
                    // hh = 1 holds (partner's odd, own odd)
                    const auto w0 = __builtin_amdgcn_permlane32_swap(e0, o0, false, false);
                    const auto w1 = __builtin_amdgcn_permlane32_swap(e1, o1, false, false);
                    const u32x4 out = {w0[0], w1[0], w0[1], w1[1]};
                    if (qr < a.n_q)
                        *reinterpret_cast<u32x4*>(obase + ((size_t)qr * a.o_rs + 32 * dt + 16 * cp + 8 * hh) * 2) = out;
                }
        }
        stamp(31);
    }
}

template <typename T, bool DBG>
__global__ void __launch_bounds__(256) attn32_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // Work item = (crop, head).  Items < n_full are one workgroup each; every later item is cut into `split` workgroups by query
    // blocks (each stages the whole K/V panel).  The cut items come last and part-major (the parts of one item are n_cut ids
    // apart: same XCD, i.e. same L2, when n_cut is a multiple of 8), so that they fill the tail of the launch: 320 items on 256
    // CUs are one round of 256 whole items + 64 items x 4 quarter-size workgroups instead of a second round that is 3/4 empty.
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int total = (a.n_q + 31) >> 5;
    const int w = blockIdx.x;
    int item, part, parts;
    if (w < a.n_full) { item = w; part = 0; parts = 1; }
    else { const int r = w - a.n_full; part = r / a.n_cut; item = a.n_full + r % a.n_cut; parts = a.split; }
    const int h = item % a.heads, b = item / a.heads;
    const int wg0 = (int)((long)total * part / parts);
    const int nblk = (int)((long)total * (part + 1) / parts) - wg0;                  // <= 20
    const int base = nblk / 4, rem = nblk % 4;
    const int cnt = base + (wave < rem ? 1 : 0);
    const int blk0 = wg0 + wave * base + min(wave, rem);
    switch (cnt) {
        case 0: attn32_body<T, 0, DBG>(a, smem, b, h, blk0); break;
        case 1: attn32_body<T, 1, DBG>(a, smem, b, h, blk0); break;
        case 2: attn32_body<T, 2, DBG>(a, smem, b, h, blk0); break;
        case 3: attn32_body<T, 3, DBG>(a, smem, b, h, blk0); break;
        case 4: attn32_body<T, 4, DBG>(a, smem, b, h, blk0); break;
        default: attn32_body<T, 5, DBG>(a, smem, b, h, blk0); break;
    }
}

// Cost model of one workgroup in kilocycles (measured: ~7.5 to stage the panel, ~0.44 per (block, step) of the busiest wave)
static double attn32_wg_cost(int total_blocks, int parts, int steps) {
    const int nblk = (total_blocks + parts - 1) / parts, nb = (nblk + 3) / 4;
    return 7.5 + 3.0 + 0.44 * nb * steps;
}

template <typename T>
static int launch_attn32(const AttnArgs& a0, int batch, int force_split, hipStream_t stream) {
    AttnArgs a = a0;
    constexpr int LDS = 2 * 608 * 128;
    const int total = (a.n_q + 31) / 32, steps = (a.n_kv + 31) / 32;
    SLIME_REQUIRE(total <= 20 * 4, "attention32: %d queries exceed 4 workgroups x 20 blocks", a.n_q);
    const int min_split = (total + 19) / 20;                  // <= 5 blocks per wave, 4 waves
    const int items = a.heads * batch, cus = num_cus();
    // whole rounds of uncut items, then the remainder cut so that it costs least: rounds(L * s) * cost(s)
    int n_full = 0, split = min_split;
    if (force_split > 0) split = max(min_split, force_split);
    else if (force_split == 0 && min_split == 1) {
        n_full = items / cus * cus;
        const int left = items - n_full;
        double best = 1e30;
        for (int s = 1; s <= 5 && left > 0; ++s) {
            if ((total + s - 1) / s < 1) break;
            const double c = (double)((left * s + cus - 1) / cus) * attn32_wg_cost(total, s, steps);
            if (c < best - 1e-9) { best = c; split = s; }
        }
        if (left == 0) split = 1;
    }
    a.n_full = n_full; a.split = split; a.n_cut = items - n_full;
    const dim3 grid(n_full + a.n_cut * split);
#ifdef SLIME_DIAG
    if (a.dbg) {
        auto kern = attn32_kernel<T, true>;
        SLIME_SET_LDS_ONCE(kern, LDS, "attention");
        hipLaunchKernelGGL(kern, grid, dim3(256), LDS, stream, a);
        SLIME_CHECK_LAUNCH("attention32");
        return SLIME_OK;
    }
#endif
    auto kern = attn32_kernel<T, false>;
    SLIME_SET_LDS_ONCE(kern, LDS, "attention");
    hipLaunchKernelGGL(kern, grid, dim3(256), LDS, stream, a);
    SLIME_CHECK_LAUNCH("attention32");
    return SLIME_OK;
}
