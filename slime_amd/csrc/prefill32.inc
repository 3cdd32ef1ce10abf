// prefill32.inc -- causal GQA prefill attention (head_dim 128, 4 query heads per kv head: Llama-3) as ONE wave per SIMD on
// 32x32x16 MFMAs.  Included by prefill.hip (shares PrefillArgs).  The CLIP kernel of the same school (attention32.inc) is bound by
// v_exp_f32 as much as by the matrix pipe; at head_dim 128 a (32-query, 32-key) block is 16 useful MFMAs for the same 16 exps, so
// the stream is matrix-pipe bound and the hand-placed softmax (slots32.h) costs nothing.
//
// Work item = (sequence, kv head, 64 query rows), a workgroup walks several (below); wave w = query head 4 kvh + w, two 32-row
// blocks per wave (160 accumulator registers in AGPRs).  Keys are walked in steps of 32 from the sequence's first token up to the diagonal; K and V of a step
// (8 + 8 KiB) travel by LDS-DMA into a ring of 8 steps, 6 steps ahead of their use: every step starts with a counted vmcnt (the
// steps t and t+1 of this wave's pieces have landed), one barrier, and the DMAs of step t+6 into the slot of step t-2.  K rows are
// 16-B-chunk XOR-swizzled (chunk ^ (row & 15): conflict-free ds_read_b128 over 32 rows of 256 B), V rows 64-B-granule swizzled
// (granule ^ (row & 3): the 4 rows x 8 pieces a half-wave transpose read touches cover all 64 banks); both swizzles are applied to
// the per-lane SOURCE address of the DMA (its LDS side is lane-linear).
//
// Pipeline (as attention32.inc): iteration (step t, block b) issues the MFMAs of QK for the next block in flattened order and of
// PV for the previous one around the speculative softmax of (t, b): 9 + 10 = 19 MFMAs = 608 matrix-pipe cycles per iteration, 16 of
// them useful.  Steps that need a mask -- the first (tokens before the sequence's start), the diagonal ones (keys after the
// query), the last of the token range -- get it applied to the finished score tile in front of the iteration; query rows outside
// the token range come out as zeros.  Scores arrive in log2 units (q carries dh^-0.5 * log2 e, as for the other kernels).

#include "slots32.h"

// Round 3: the kernel is PERSISTENT over work items.  The items are numbered heaviest first (L = kvh + n_kv (b + batch z), query
// block nqb - 1 - z); a grid of G workgroups (one per CU: the 128 KiB ring allows no second one) walks them in snake order
// (round r: item r G + w, odd rounds mirrored inside the workgroup's XCD class).  For the arithmetic progression of causal lengths
// that IS the longest-processing-time schedule, and it needs no counter: concurrent launches share nothing.  What the loop buys
// is the seam between items: the K/V ring does not stop at an item's last step -- the look-ahead DMAs that used to fetch six
// ignored steps fetch the first six steps of the workgroup's NEXT item (the generator below walks the items on its own, six steps
// ahead of the consumer), the next item's Q rows are requested in front of the finished item's drain / normalise / store, and no
// workgroup is launched between items.  With G = the number of items it is the round-2 kernel (diagnostic variant 2; bit-equal:
// tests/test_gpu_prefill.py).  Ring bookkeeping: an item advances the ring by its step count rounded up to even (the main loop
// is written in pairs of steps), generator and consumer alike.
// Measured (tools/prefill_stamps.py, s_memtime; profiles/r03_prefill_stamps.txt): with one item per workgroup 24 % of a
// workgroup's life at 8 x 1216 (config 4: 1216 items of 2..38 steps, 4.75 per CU) was start-up -- launch, first DMAs and Q cold --
// and the 3 masked steps of an item cost 1.5x a plain one.  Persistent: start-up 3.5 %, main loop 73 %, the rest per item
// (prologue 3.4k, drain / normalise / store 5.9k, next item + Q request 2.6k ticks against 2.0k per step); kernel 0.146-0.166 ->
// 0.137-0.145 ms, same box (8 x 700: 0.060 -> 0.055; 1 x 9280 and 4 x 4096: +-2 %).  What is left of the gap to the long-sequence
// rate is those per-item costs (a 64-row item at S = 1216 is only 20 steps long) and the static schedule's tail (98 steps on the
// fullest workgroup against 95 on average, 5 items against 4).  "Three 32-row blocks per wave" (VERDICT r2) does not fit: the
// two blocks already hold 160 AGPRs + 256 VGPRs (64 of them Q); a third needs 80 + 32 more.

// WIN: the sliding-window instantiation (Mistral / Mixtral: query row i sees key j iff j <= i and i - j < a.window).  An item's first
// step becomes max(ks, q_lo - W + 1) >> 5 -- generator, ring bookkeeping and consumer all take their step counts from load_item, so
// they agree by construction and behind the window every item is ceil((W + 63 + 31) / 32)-ish steps long.  The leading steps up to
// and including the one that holds the LAST row's first visible key, q_lo + 64 - W (32 st <= q_lo + 64 - W: up to three behind
// t_first), get a two-sided mask with a per-row lower bound.  The test is inclusive: q_lo is a multiple of 64, so for every W
// that is a multiple of 32 (4096, the Mistral default) that key is the FIRST key of its step, and the last row starts there.  A row whose window opens in such a step has seen no live key yet: take_reference left its reference at 0 and its
// accumulators are exact zeros, so the step it STARTS in sets the reference to its row maximum whatever the sign (the lazy rescale
// alone only ever moves up, and scores far below 0 would underflow P) and leaves the zero accumulators alone (alpha = 1: 0 x inf
// would be NaN).  Every row starts in t_first or in one of those leading steps.  WIN = false compiles the code as it was.
template <typename T, int P = 6, bool WIN = false>             // P: key steps requested ahead of their use (6; 4 = measured alternative)
__global__ void __launch_bounds__(256) prefill32_kernel(PrefillArgs a) {
    static_assert(P == 4 || P == 6, "the pair loop needs an even look-ahead of at least 4 steps inside the 8-slot ring");
    constexpr int RB = 256, NB = 2, R = 8, STEP = 32 * RB, GROUP = 4;
    constexpr float RESCALE_TH = 8.0f;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Klds = smem;
    char* Vlds = smem + R * STEP;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q31 = lane & 31, hh = lane >> 5;
    const int nqb = (a.S + 63) >> 6;

    // ---- the workgroup's items ----
    const int n_items = a.n_kv_heads * a.batch * nqb;
    const int G = (int)gridDim.x, w = (int)blockIdx.x;
    const int rounds = (n_items + G - 1) / G;
    const int wm = (G & 7) == 0 ? ((((G >> 3) - 1 - (w >> 3)) << 3) | (w & 7)) : G - 1 - w;
    struct Item { int kvh, b, q_lo, ks, ke, t_first, t_end; };     // token range [ks, ke), key steps [t_first, t_end); empty: t_end == t_first
    auto load_item = [&](int r, Item& it) __attribute__((always_inline)) -> bool {                // false: no item for this workgroup in round r
        const int L = r * G + ((r & 1) ? wm : w);
        if (L >= n_items) return false;
        it.kvh = L % a.n_kv_heads;
        const int rest = L / a.n_kv_heads;
        it.b = rest % a.batch;
        it.q_lo = (nqb - 1 - rest / a.batch) * 64;                 // heaviest (latest) blocks first
        it.ks = a.kv_start ? a.kv_start[it.b] : 0;
        it.ke = a.kv_len ? min(a.S, it.ks + a.kv_len[it.b]) : a.S;
        const int kv_hi = min(it.ke, it.q_lo + 64);                // causal: no key beyond the last query row
        it.t_first = it.ks >> 5;
        if constexpr (WIN) it.t_first = max(it.ks, it.q_lo - a.window + 1) >> 5;
        it.t_end = (kv_hi + 31) >> 5;
        if (it.t_end <= it.t_first || it.q_lo >= it.ke) it.t_end = it.t_first;    // no query row inside the token range
        return true;
    };
    // (lane-derived addresses of the code between items are recomputed there: hoisted out of the item loop they would sit in
    // registers the main loop has none to spare of)
    auto fresh_lane = [&]() __attribute__((always_inline)) { int l = lane; asm volatile("" : "+v"(l)); return l; };
    auto out_base = [&](const Item& it) __attribute__((always_inline)) { return a.o + ((size_t)it.b * a.o_bs + (size_t)(it.kvh * GROUP + wave) * 128) * 2; };
    // consumer side: the next item with work after round r; items without get their zeros here
    auto next_item = [&](int& r, Item& it) __attribute__((always_inline)) -> bool {
        for (;;) {
            if (++r >= rounds) return false;
            if (!load_item(r, it)) continue;
            if (it.t_end > it.t_first) return true;
            char* obase = out_base(it);
            const int ln = fresh_lane(), q31 = ln & 31, hh = ln >> 5;
#pragma unroll
            for (int s = 0; s < NB; ++s) {
                const int qr = it.q_lo + 32 * s + q31;
                if (qr < a.S)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        *reinterpret_cast<u32x4*>(obase + ((size_t)qr * a.o_rs + 16 * j + 8 * hh) * 2) = u32x4{0u, 0u, 0u, 0u};
            }
        }
    };

    // ---- Q: B operand of QK, lane (q, hh) holds d = 16 j + 8 hh .. + 7 of its query row for the eight d-steps j (asm loads:
    // hipcc must not count them beside the LDS-DMA stream).  ONE request site per loop iteration (no copies of registers whose
    // data is still in flight). ----
    u32x4 qf[NB][8];
    auto load_q = [&](const Item& it) __attribute__((always_inline)) {
        const char* qbase = a.q + ((size_t)it.b * a.q_bs + (size_t)(it.kvh * GROUP + wave) * 128) * 2;
        const int ln = fresh_lane(), q31 = ln & 31, hh = ln >> 5;
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            const int qr = min(it.q_lo + 32 * s + q31, a.S - 1);
            const char* qp = qbase + ((size_t)qr * a.q_rs + 8 * hh) * 2;
            asm volatile("global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %4, off offset:32\n\t"
                         "global_load_dwordx4 %2, %4, off offset:64\n\tglobal_load_dwordx4 %3, %4, off offset:96"
                         : "=&v"(qf[s][0]), "=&v"(qf[s][1]), "=&v"(qf[s][2]), "=&v"(qf[s][3]) : "v"(qp) : "memory");
            asm volatile("global_load_dwordx4 %0, %4, off offset:128\n\tglobal_load_dwordx4 %1, %4, off offset:160\n\t"
                         "global_load_dwordx4 %2, %4, off offset:192\n\tglobal_load_dwordx4 %3, %4, off offset:224"
                         : "=&v"(qf[s][4]), "=&v"(qf[s][5]), "=&v"(qf[s][6]), "=&v"(qf[s][7]) : "v"(qp) : "memory");
        }
    };

    // ---- K/V ring: a step is 8 K pieces + 8 V pieces of 1 KiB (4 rows of 256 B); wave w moves pieces 2 w, 2 w + 1 of both.  The
    // GENERATOR walks the workgroup's items by itself: running source pointers, one per (operand, piece of this wave) -- a step
    // further is 32 rows further (no multiplies in the loop), rows past the sequence are clamped to its last row by a select
    // (masked, or never used) -- and a running ring offset; when an item's (even-padded) steps are all requested it moves the
    // pointers to the next item with work.  Past the last item it keeps requesting clamped rows (ignored; the counts stay constants).
    const char* kp[2]; const char* vp[2]; const char* klast[2]; const char* vlast[2];
    int drow[2];                                               // row the pointers of piece u point at
    const long kstride = (long)a.k_rs * 64, vstride = (long)a.v_rs * 64;      // 32 rows in bytes
    int gen_r = -1, gen_left = 0;
    unsigned gslot = 0;                                        // ring byte offset of the step requested next
    auto gen_next = [&]() __attribute__((always_inline)) {
        Item it;
        for (;;) {
            if (++gen_r >= rounds) { gen_left = 0x40000000; return; }      // (even, and never reaches 0)
            if (load_item(gen_r, it) && it.t_end > it.t_first) break;
        }
        gen_left = (it.t_end - it.t_first + 1) & ~1;
        const char* kbase = a.k + ((size_t)it.b * a.k_bs + (size_t)it.kvh * 128) * 2;
        const char* vbase = a.v + ((size_t)it.b * a.v_bs + (size_t)it.kvh * 128) * 2;
        const int ln = fresh_lane();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int lr = (2 * wave + u) * 4 + (ln >> 4), cpos = ln & 15;
            const unsigned ksw = (cpos ^ (lr & 15)) << 4, vsw = (cpos ^ ((lr & 3) << 2)) << 4;
            drow[u] = it.t_first * 32 + lr;
            kp[u] = kbase + (size_t)drow[u] * a.k_rs * 2 + ksw;
            vp[u] = vbase + (size_t)drow[u] * a.v_rs * 2 + vsw;
            klast[u] = kbase + (size_t)(a.S - 1) * a.k_rs * 2 + ksw;
            vlast[u] = vbase + (size_t)(a.S - 1) * a.v_rs * 2 + vsw;
        }
    };
    auto dma_half = [&](int u) __attribute__((always_inline)) {                               // pieces 2 wave + u of K and V of the generator's step
        const int piece = 2 * wave + u;
        const bool inside = drow[u] < a.S;
        __builtin_amdgcn_global_load_lds(GLOBAL_PTR(inside ? kp[u] : klast[u]), LDS_PTR(Klds + gslot + piece * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(GLOBAL_PTR(inside ? vp[u] : vlast[u]), LDS_PTR(Vlds + gslot + piece * 1024), 16, 0, 0);
        kp[u] += kstride; vp[u] += vstride; drow[u] += 32;
        if (u == 1) gslot = (gslot + STEP) & (R * STEP - 1);
    };
    // after every PAIR of requested steps (items are even-padded, so an item ends on a pair): keeps the item switch -- divisions,
    // 64-bit address products -- out of the MFMA-dense iterations
    auto gen_pair_done = [&]() __attribute__((always_inline)) {
        gen_left -= 2;
        if (__builtin_expect(gen_left == 0, 0)) gen_next();
    };
    // Top of a PAIR of steps (t, t+1): this wave's pieces of the steps t, t+1, t+2 have landed (K of step t+2 is requested during
    // step t+1) when at most the 12 DMAs of the steps t+3..t+5 still fly; everybody's after the barrier.  The slots of the steps
    // t-2 and t-1 -- nobody reads them any more -- are refilled with the steps t+6 and t+7 from inside the four iterations that
    // follow (one K piece + one V piece behind the last filler of each), so that the issue cost of a DMA (~60-100 cycles in which
    // the wave issues nothing else) falls where the matrix pipe has work queued.  (Steps count along the ring, across items.)
    auto pair_top = [&]() __attribute__((always_inline)) {
        if constexpr (P == 6) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");    // (only step t+3 may still fly)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    f32x16 o[NB][4], osum[NB];
    float m_ref[NB];
    u32x4 qx[NB];
    // the item the consumer works on
    int ks_ = 0, ke_ = 0, q_lo = 0, t_first = 0, t_end = 0, t_diag = 0;
    int lim[NB];
    char* obase = nullptr;
    const unsigned one2 = T::pack2(1.0f, 1.0f);
    u32x4 ones = {one2, one2, one2, one2};
    // reference k-step: -m_ref travels as THREE 16-bit terms (slots 0..2 of the B operand against ones in the A operand), i.e.
    // exactly: language-model logits reach 1e6 and more, where a single bf16 term would be off by thousands of log2 units
    u32x4 kx = {hh == 0 ? T::pack2(1.0f, 1.0f) : 0u, hh == 0 ? T::pack2(1.0f, 0.0f) : 0u, 0u, 0u};
    auto set_reference = [&](u32x4& q, float m) __attribute__((always_inline)) {             // q <- B operand carrying -m
        const float x = -m;
        const unsigned w0 = T::pack2(x, 0.0f);
        const float r1 = x - T::lo(w0);
        const unsigned w1 = T::pack2(r1, 0.0f);
        const float r2 = r1 - T::lo(w1);
        const unsigned w2 = T::pack2(r2, 0.0f);
        q[0] = hh == 0 ? ((w0 & 0xffffu) | (w1 << 16)) : 0u;
        q[1] = hh == 0 ? (w2 & 0xffffu) : 0u;
        asm volatile("" : "+v"(q));
    };
    float th = RESCALE_TH;
    asm volatile("" : "+v"(ones), "+v"(kx), "+v"(th));
    // LDS addresses inside a slot
    unsigned kb[8], vb[4];
#pragma unroll
    for (int j = 0; j < 8; ++j) kb[j] = lds_byte_addr(Klds) + q31 * RB + (((2 * j + hh) ^ (q31 & 15)) << 4);
    {
        const int dblk = (lane >> 4) & 1, i16 = lane & 15, pa = i16 & 3, bb = i16 >> 2;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) vb[dt] = lds_byte_addr(Vlds) + (4 * hh + bb) * RB + ((dt ^ bb) << 6) + (4 * dblk + pa) * 8;
    }
    // masks: key kv (32 t + (r & 3) + 8 (r >> 2) + 4 hh) is live for query row qrow iff ks_ <= kv <= min(ke_ - 1, qrow);
    // lim[s] = qrow, or -1 for rows outside the token range (nothing is live); t_diag = first step with a key beyond some query
    // row of the item
    auto apply_mask = [&](f32x16& t, int step, int blk) __attribute__((always_inline)) {
        // element r holds key 32 step + 4 hh + (r & 3) + 8 (r >> 2).  Upper bound (causal, end of the token range, rows outside
        // the range: lim = -1): offset <= d, one compare + one select per element.  The lower bound only exists in a range's
        // first step when the range does not start on a step boundary (left padding): a uniform, rare branch.
        int d = lim[blk] - (step * 32 + 4 * hh);
        asm volatile("" : "+v"(d));                           // opaque: hipcc otherwise hoists the compares of a mask into the
                                                              // unmasked path of every iteration
        bool two_sided = ks_ > step * 32;
        if constexpr (WIN) two_sided = two_sided || step * 32 <= q_lo + 64 - a.window;       // (uniform: the item's last row's edge)
        if (__builtin_expect(two_sided, 0)) {
            int lo = ks_ - (step * 32 + 4 * hh);
            if constexpr (WIN) lo = max(ks_, lim[blk] - a.window + 1) - (step * 32 + 4 * hh); // per row (lim = -1: d < 0, all dead)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int off = (r & 3) + 8 * (r >> 2);
                t[r] = (off >= lo && off <= d) ? t[r] : -INFINITY;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = ((r & 3) + 8 * (r >> 2) <= d) ? t[r] : -INFINITY;
        }
    };

    u32x4 kf[8];
    u32x2 vr[4][2][2];                                        // V^T fragments [d-tile][kv half j][slot half c]
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int j = 0; j < 2; ++j) { vr[dt][j][0] = u32x2{0u, 0u}; vr[dt][j][1] = u32x2{0u, 0u}; }
#define P32_VR_ALL "v"(vr[0][0][0]), "v"(vr[0][0][1]), "v"(vr[0][1][0]), "v"(vr[0][1][1]), "v"(vr[1][0][0]), "v"(vr[1][0][1]), \
                   "v"(vr[1][1][0]), "v"(vr[1][1][1]), "v"(vr[2][0][0]), "v"(vr[2][0][1]), "v"(vr[2][1][0]), "v"(vr[2][1][1]), \
                   "v"(vr[3][0][0]), "v"(vr[3][0][1]), "v"(vr[3][1][0]), "v"(vr[3][1][1])
#define P32_KF_ALL "v"(kf[0]), "v"(kf[1]), "v"(kf[2]), "v"(kf[3]), "v"(kf[4]), "v"(kf[5]), "v"(kf[6]), "v"(kf[7])
    unsigned cons_base = 0;                                    // ring byte offset of the consumer's item's first step
    unsigned kslot = 0;                                        // byte offset of the slot the NEXT K request reads
    unsigned vslot = 0;                                        //                              ... the next V request
    auto k_request1 = [&](int j) __attribute__((always_inline)) { kf[j] = lds32_b128<0>(kb[j] + kslot); };
    auto k_advance = [&]() __attribute__((always_inline)) { kslot = (kslot + STEP) & (R * STEP - 1); };
    auto v_request0 = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { vr[dt][0][0] = lds32_tr16<0>(vb[dt] + vslot); vr[dt][0][1] = lds32_tr16<8 * RB>(vb[dt] + vslot); }
    };
    auto v_request1 = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { vr[dt][1][0] = lds32_tr16<16 * RB>(vb[dt] + vslot); vr[dt][1][1] = lds32_tr16<24 * RB>(vb[dt] + vslot); }
        vslot = (vslot + STEP) & (R * STEP - 1);
    };

    f32x16 S[2];
    u32x4 pf[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p) { pf[p][0] = u32x4{0u, 0u, 0u, 0u}; pf[p][1] = u32x4{0u, 0u, 0u, 0u}; }

    // ---- one step = two iterations of the pipeline ----
    auto step = [&](const int st) __attribute__((always_inline)) {                            // its second iteration requests one more step of the ring
        bool masked = st == t_first || st >= t_diag;
        bool win_lead = false;                                 // a leading step behind t_first in which rows may start (WIN only)
        if constexpr (WIN) { win_lead = st > t_first && st * 32 <= q_lo + 64 - a.window; masked = masked || win_lead; }
#pragma unroll
        for (int s = 0; s < NB; ++s)                          // (the accumulators stay in the AGPR file across every edge of the loop nest)
            asm volatile("" : "+a"(o[s][0]), "+a"(o[s][1]), "+a"(o[s][2]), "+a"(o[s][3]), "+a"(osum[s]));
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) {
            const int fp = blk & 1, pb = blk ^ 1, nb = blk ^ 1;          // previous / next block in flattened order (NB = 2)
            const bool last = blk == NB - 1;
            f32x16& sc = S[fp];
            f32x16& sn = S[fp ^ 1];
            if (__builtin_expect(masked, 0)) {
                apply_mask(sc, st, blk);
                asm volatile("" : "+v"(sc));
            }
            float e[16], m0, m1, m2, m3, m4;
            unsigned pk[8];
            unsigned long long runaway = 0;
            // pair i: MFMA A = k-step i of QK(next) into sn (i = 8: the reference step), MFMA B = MFMA i of PV(prev)
            //         PV MFMA idx: 5 j + w, w = 0..3 the O^T d-tiles, w = 4 the row sums
            auto pair = [&](int i) __attribute__((always_inline)) {
                const int ka = i == 0 ? 1 : 2;
                f32x16& sv = sn;
                const u32x4 ma = i < 8 ? kf[i] : kx, mb = i < 8 ? qf[nb][i] : qx[nb];
                const int j = i / 5, w = i % 5;
                f32x16& av = w == 4 ? osum[pb] : o[pb][w & 3];
                const u32x4 vfw = {vr[w & 3][j][0][0], vr[w & 3][j][0][1], vr[w & 3][j][1][0], vr[w & 3][j][1][1]};
                const u32x4 mab = w == 4 ? ones : vfw, mbb = pf[fp ^ 1][j];
                switch (i) {
                    case 0: A32_PAIR(P01); break;
                    case 1: A32_PAIR(P23); break;
                    case 2: A32_PAIR(P45); break;
                    case 3: A32_PAIR(P67); break;
                    case 4: A32_PAIR(P89); break;
                    case 5: A32_PAIR(P10P); break;
                    default:
                        asm volatile(A32_MF_AC A32_MFB : [acc] "+v"(sv), [accb] "+a"(av) : [ma] "v"(ma), [mb] "v"(mb), [mab] "v"(mab), [mbb] "v"(mbb));
                        break;
                }
            };
            // LDS queue at the top of iteration 1: [K 0..6][V half 0 x 8][K 7][V half 1 x 8]
            if (last) A32_WAIT("lgkmcnt(9)", P32_KF_ALL, P32_VR_ALL);
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                if (last && i == 5) A32_WAIT("lgkmcnt(0)", P32_KF_ALL, P32_VR_ALL);
                pair(i);
                // requests go where the gaps hold no softmax work (pairs 6..8): K fragment j of the next step any time after
                // pair j, V half 0 after MFMA 4 of PV(st-1, 1)
                if (!last && i == 5) { k_request1(0); k_request1(1); k_request1(2); }
                if (!last && i == 6) { k_request1(3); k_request1(4); k_request1(5); k_request1(6); v_request0(); }
                if (!last && i == 7) k_request1(7);
                if (last && i == 6) dma_half(0);               // behind the last filler
                if (last && i == 7) dma_half(1);
            }
            {
                f32x16& av = osum[pb];
                const u32x4 mab = ones, mbb = pf[fp ^ 1][1];
                asm volatile(A32_MFB : [accb] "+a"(av) : [mab] "v"(mab), [mbb] "v"(mbb));
            }
            if (!last) { v_request1(); k_advance(); }
            if (__builtin_expect(runaway != 0 || win_lead, 0)) {
                float mx = sc[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) mx = __builtin_fmaxf(mx, sc[r]);
                const unsigned u = __float_as_uint(mx);
                const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
                // only the rows that ran away themselves move (a row's result must not depend on what shares its block: changing
                // LATER tokens may not change earlier rows by a bit); for the others d = 0 reproduces the speculative values
                float d = __builtin_fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
                bool starting = false;
                if constexpr (WIN) {                           // this row's first live key lies in this step: its reference is this maximum
                    const int first_key = max(ks_, lim[blk] - a.window + 1);
                    starting = win_lead && lim[blk] >= 0 && first_key >= st * 32 && first_key < st * 32 + 32;
                }
                d = (d > RESCALE_TH || starting) ? d : 0.f;
                m_ref[blk] += d;
                set_reference(qx[blk], m_ref[blk]);
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    pk[q] = T::pack2(__builtin_amdgcn_exp2f(sc[2 * q] - d), __builtin_amdgcn_exp2f(sc[2 * q + 1] - d));
                const float alpha = starting ? 1.0f : __builtin_amdgcn_exp2f(-d);     // (a starting row's accumulators are zeros)
                asm volatile("s_nop 7\n\ts_nop 7" : "+a"(o[blk][0]), "+a"(o[blk][1]), "+a"(o[blk][2]), "+a"(o[blk][3]), "+a"(osum[blk]));
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    o[blk][0][r] *= alpha; o[blk][1][r] *= alpha; o[blk][2][r] *= alpha; o[blk][3][r] *= alpha; osum[blk][r] *= alpha;
                }
                asm volatile("" : "+a"(o[blk][0]), "+a"(o[blk][1]), "+a"(o[blk][2]), "+a"(o[blk][3]), "+a"(osum[blk]));
            }
            pf[fp][0] = u32x4{pk[0], pk[1], pk[2], pk[3]};
            pf[fp][1] = u32x4{pk[4], pk[5], pk[6], pk[7]};
            asm volatile("" : "+v"(pf[fp][0]), "+v"(pf[fp][1]));
        }
#pragma unroll
        for (int s = 0; s < NB; ++s)
            asm volatile("" : "+a"(o[s][0]), "+a"(o[s][1]), "+a"(o[s][2]), "+a"(o[s][3]), "+a"(osum[s]));
    };

    auto qk8 = [&](int blk) __attribute__((always_inline)) {
        f32x16& t = S[blk & 1];
        Mfma32Asm<T>::first(t, kf[0], qf[blk][0]);
#pragma unroll
        for (int j = 1; j < 8; ++j) Mfma32Asm<T>::next(t, kf[j], qf[blk][j]);
    };
    auto take_reference = [&](int blk) __attribute__((always_inline)) {
        f32x16& t = S[blk & 1];
        apply_mask(t, t_first, blk);
        float mx = max3f(t[0], t[1], t[2]);
        mx = max3f(mx, t[3], t[4]); mx = max3f(mx, t[5], t[6]); mx = max3f(mx, t[7], t[8]); mx = max3f(mx, t[9], t[10]);
        mx = max3f(mx, t[11], t[12]); mx = max3f(mx, t[13], t[14]); mx = __builtin_fmaxf(mx, t[15]);
        const unsigned u = __float_as_uint(mx);
        const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        mx = __builtin_fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        mx = mx == -INFINITY ? 0.f : mx;                       // a row with no live key in the first step is outside the token range
        m_ref[blk] = mx;
        set_reference(qx[blk], mx);
    };

#ifdef SLIME_DIAG
    // diagnostic build: where a workgroup's time goes (s_memtime ticks summed over workgroups into a.dbg[0..7]: start-up, item
    // prologue, main loop, next item + Q request, drain / normalise / store, wait for Q, steps, items)
    unsigned long long dbg_t[6] = {0, 0, 0, 0, 0, 0}, dbg_last = __builtin_amdgcn_s_memtime();
    unsigned dbg_steps = 0, dbg_items = 0;
#define P32_STAMP(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); dbg_t[k] += t_ - dbg_last; dbg_last = t_; } while (0)
#else
#define P32_STAMP(k) do { } while (0)
#endif
    // ---- one item, from its Q rows in flight to the end of its last step (the PV of the last block stays in the pipeline) ----
    // Q has landed -- and with it everything older in the queue: the look-ahead DMAs (the item's first six steps; requested at
    // least three steps ago) and the previous item's stores.  The counted waits of the pairs that follow are then merely
    // conservative on top of an empty queue.  (Stands at the END of the loop body: copies the register allocator may place on the
    // back edge for the Q registers then read landed data.)
    auto wait_q = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            A32_WAIT("vmcnt(0)", "v"(qf[s][0]), "v"(qf[s][1]), "v"(qf[s][2]), "v"(qf[s][3]));
            A32_WAIT("vmcnt(0)", "v"(qf[s][4]), "v"(qf[s][5]), "v"(qf[s][6]), "v"(qf[s][7]));
        }
    };
    auto item_body = [&](const Item& it) __attribute__((always_inline)) {
        ks_ = it.ks; ke_ = it.ke; q_lo = it.q_lo; t_first = it.t_first; t_end = it.t_end;
        t_diag = q_lo >> 5;
        obase = out_base(it);
        kslot = cons_base; vslot = cons_base;
        cons_base = (cons_base + (unsigned)((t_end - t_first + 1) & ~1) * STEP) & (R * STEP - 1);
        const int lq31 = fresh_lane() & 31;
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            const int qrow = q_lo + 32 * s + lq31;
            lim[s] = (qrow >= ks_ && qrow < ke_) ? qrow : -1;
            m_ref[s] = 0.f;
            qx[s] = u32x4{0u, 0u, 0u, 0u};
            asm volatile("" : "+v"(qx[s]));
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[s][0][r] = 0.f; o[s][1][r] = 0.f; o[s][2][r] = 0.f; o[s][3][r] = 0.f; osum[s][r] = 0.f; }
            asm volatile("" : "+a"(o[s][0]), "+a"(o[s][1]), "+a"(o[s][2]), "+a"(o[s][3]), "+a"(osum[s]));
        }
        // the first iteration's PV adds P = 0 times whatever the V^T registers hold: keep that finite
#pragma unroll
        for (int p = 0; p < 2; ++p) { pf[p][0] = u32x4{0u, 0u, 0u, 0u}; pf[p][1] = u32x4{0u, 0u, 0u, 0u}; }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int j = 0; j < 2; ++j) { vr[dt][j][0] = u32x2{0u, 0u}; vr[dt][j][1] = u32x2{0u, 0u}; }
        asm volatile("s_barrier" ::: "memory");               // everybody's pieces; everybody is done with the previous item's slots
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 8; ++j) k_request1(j);
        k_advance();
        A32_WAIT("lgkmcnt(0)", P32_KF_ALL);
        qk8(1);
        qk8(0);                                                // 8 MFMAs behind the tile read next
        asm volatile("" : "+v"(S[1]));
        take_reference(1);
        asm volatile("s_nop 7\n\ts_nop 7" : "+v"(S[0]));
        take_reference(0);
#pragma unroll
        for (int r = 0; r < 16; ++r) S[0][r] -= m_ref[0];      // (masked entries stay -inf; step() masks again, harmlessly)
        asm volatile("" : "+v"(S[0]));

#ifdef SLIME_DIAG
        P32_STAMP(1);
        dbg_steps += (unsigned)(t_end - t_first); ++dbg_items;
#endif
        for (int st = t_first; st < t_end; st += 2) {
            if (st > t_first) pair_top();
            step(st);
            if (st + 1 < t_end) step(st + 1);
            else { dma_half(0); dma_half(1); }                 // the ring moves in pairs of steps
            gen_pair_done();
        }
    };

    // ---- the end of an item: PV of the last block (its P is in pf[1], V^T of the last step in the fragment registers), normalise,
    // store.  Runs AFTER the next item's Q rows have been requested; the consumer's
    // variables (q_lo, lim, obase) still describe the finished item. ----
    auto item_finish = [&]() __attribute__((always_inline)) {
        A32_WAIT("lgkmcnt(0)", P32_VR_ALL, P32_KF_ALL);
        {
            u32x4 p0 = pf[1][0], p1 = pf[1][1];
            asm volatile("s_nop 3" : "+v"(p0), "+v"(p1));
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const u32x4 vfw = {vr[dt][j][0][0], vr[dt][j][0][1], vr[dt][j][1][0], vr[dt][j][1][1]};
                    Mfma32Asm<T>::run(o[1][dt], vfw, j == 0 ? p0 : p1);
                }
                Mfma32Asm<T>::run(osum[1], ones, j == 0 ? p0 : p1);
            }
        }
        asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
#pragma unroll
        for (int s = 0; s < NB; ++s)
            asm volatile("" : "+a"(o[s][0]), "+a"(o[s][1]), "+a"(o[s][2]), "+a"(o[s][3]), "+a"(osum[s]));

        // lane (q, hh) holds d = 32 dt + 8 c + 4 hh + 0..3: a half swap between the lane pair makes that 8 consecutive d -> 16-B stores
        const int ln = fresh_lane(), q31 = ln & 31, hh = ln >> 5;
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            const int qr = q_lo + 32 * s + q31;
            const bool whole = q_lo + 32 * s + 32 <= a.S;          // every row of the block exists
            // rows outside the token range: every P was 0, so o = +0 (and the row sum, hence 0 x (1 / 0) = NaN without the select)
            const float inv = lim[s] >= 0 ? 1.0f / osum[s][0] : 0.0f;
            char* rowp = obase + ((size_t)qr * a.o_rs + 8 * hh) * 2;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int cp = 0; cp < 2; ++cp) {
                    const int ce = 2 * cp, co = 2 * cp + 1;
                    unsigned e0 = T::pack2(o[s][dt][4 * ce] * inv, o[s][dt][4 * ce + 1] * inv);
                    unsigned e1 = T::pack2(o[s][dt][4 * ce + 2] * inv, o[s][dt][4 * ce + 3] * inv);
                    unsigned o0 = T::pack2(o[s][dt][4 * co] * inv, o[s][dt][4 * co + 1] * inv);
                    unsigned o1 = T::pack2(o[s][dt][4 * co + 2] * inv, o[s][dt][4 * co + 3] * inv);
                    const auto w0 = __builtin_amdgcn_permlane32_swap(e0, o0, false, false);
                    const auto w1 = __builtin_amdgcn_permlane32_swap(e1, o1, false, false);
                    const u32x4 out = {w0[0], w1[0], w0[1], w1[1]};
                    u32x4* dst = reinterpret_cast<u32x4*>(rowp + (32 * dt + 16 * cp) * 2);
                    if (whole) *dst = out;                         // (uniform: no exec juggling around each of the 16 stores)
                    else if (qr < a.S) *dst = out;
                }
        }
    };

    // ---- the workgroup's items ----
    Item cur;
    int cr = -1;
    gen_next();                                                // (a workgroup without any item with work would request clamped rows of
    if (gen_r >= rounds) {                                     //  nothing: leave before the first DMA; its empty items still get their zeros)
        while (next_item(cr, cur)) {}
        return;
    }
#pragma unroll
    for (int i = 0; i < P / 2; ++i) { dma_half(0); dma_half(1); dma_half(0); dma_half(1); gen_pair_done(); }
    next_item(cr, cur);                                        // the item the generator found
    load_q(cur);
    wait_q();
    P32_STAMP(0);
    for (bool more = true; more;) {
        item_body(cur);
        P32_STAMP(2);
        more = next_item(cr, cur);
        if (more) load_q(cur);                                 // the next item's Q rows fly under this item's drain / normalise / store
        P32_STAMP(3);
        item_finish();
        P32_STAMP(4);
        if (more) wait_q();
        P32_STAMP(5);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the look-ahead DMAs must not outlive the workgroup's LDS
#ifdef SLIME_DIAG
    if (a.dbg && tid == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicAdd(a.dbg + k, dbg_t[k]);
        atomicAdd(a.dbg + 6, (unsigned long long)dbg_steps);
        atomicAdd(a.dbg + 7, (unsigned long long)dbg_items);
    }
#endif
#undef P32_STAMP
#undef P32_VR_ALL
#undef P32_KF_ALL
}
