// gemm_diag.inc -- everything of the GEMM that exists in the DIAGNOSTIC build only (libslime_hip_diag.so, -DSLIME_DIAG: tools/ and
// the tile-forcing tests).  Included by gemm.hip under SLIME_DIAG, after the product kernels and launchers and before launch_epi.
//   * the process-global tuning / ablation hooks and their setters;
//   * the measured-alternative kernels gemm_ppp_kernel (persistent ping-pong) and gemm_pp32b_kernel (32x32x16 MFMAs), the 192-row
//     ping-pong launcher and the declarations of gemm_ps.hip's persistent direct-B kernels;
//   * the timing ablations of the ping-pong and stream kernels;
//   * diag_launch_epi, the one call launch_epi makes into this file, and diag_hook_args, the one slime_gemm_ex makes.
#include <optional>

// Process-global tuning / ablation hooks.  The product library has no mutable global state: its dispatch is a pure function of
// the shape.
static int g_ablation = 0;
static int g_group_m = 0;
static unsigned long long* g_dbg = nullptr;
extern "C" void slime_gemm_set_debug(void* p) { g_dbg = (unsigned long long*)p; }
extern "C" void slime_gemm_set_ablation(int a) { g_ablation = a; }
extern "C" void slime_gemm_set_group_m(int s) { g_group_m = s; }
static int g_db_abl = 0;
extern "C" void slime_gemm_set_db_ablation(int a) { g_db_abl = a; }
static int g_force_tile = 0;   // 0 = auto_tile()
static int g_sched = 1;        // 0 = compiler schedule, 1 = pinned software pipeline (lock-step kernels)
extern "C" void slime_gemm_force_tile(int t) { g_force_tile = t; }
extern "C" void slime_gemm_set_sched(int s) { g_sched = s; }
// per-shape tile override table (N, K) -> tile, consulted in auto mode; tile 0 clears the table
static int g_rule_n[8], g_rule_k[8], g_rule_tile[8], g_rules = 0;
extern "C" void slime_gemm_set_shape_tile(int N, int K, int tile) {
    if (tile == 0) { g_rules = 0; return; }
    for (int i = 0; i < g_rules; ++i)
        if (g_rule_n[i] == N && g_rule_k[i] == K) { g_rule_tile[i] = tile; return; }
    if (g_rules < 8) { g_rule_n[g_rules] = N; g_rule_k[g_rules] = K; g_rule_tile[g_rules] = tile; ++g_rules; }
}
// epilogues the 96-row direct-B tile (tile 19) is built for: the tower's three, for the per-shape A/B tools (tools/r6_tile_ab.py,
// r6_small_tiles.py).  Every other epilogue keeps 128 rows.
constexpr bool db96_epilogue(int epi) {
    return epi == SLIME_EPI_BIAS_T || epi == SLIME_EPI_BIAS_QUICKGELU_T || epi == SLIME_EPI_BIAS_RESID_SPLIT_LN;
}

// ================================================================================================
// Persistent ping-pong kernel: the ping-pong kernel above, but a workgroup walks its output tiles
// (tile = blockIdx.x, + gridDim.x, ...) as ONE continuous k-tile stream.
//
// Why (s_memtime stamps, 256x256 tiles at K = 1024): a one-tile workgroup spends 2.8k cycles in its
// prologue (first DMA latency), 43k in the main loop and 9-13k in the epilogue, and because all CUs run
// in lock step the 256 x 128..256 KB of epilogue stores hit HBM as one burst while the memory system
// idles during main loops.  Here
//   * the LDS-DMA schedule never drains between tiles: "tile t+1 / t+2" of the issue table simply
//     runs into the next output tile, so its k-tiles 0/1 are already in LDS when the current tile ends;
//   * the epilogue only ISSUES its stores; they drain under the next tile's MFMAs.  vmcnt counts stores
//     too and loads/stores may retire out of order with respect to each other, so counted waits are
//     only used where nothing older than the wanted loads can be pending: the wave drains its DMA
//     (vmcnt(0)) right before the epilogue, issues the stores, skips the (unneeded) waits of the next
//     tile's first k-tile, and resumes the counted vmcnt(8) at k-tile 1 -- by then the stores have had
//     >= 4 slots plus the epilogue arithmetic to complete.
// ================================================================================================
template <typename T, int EPI, int KTAG>
__global__ void __launch_bounds__(512) gemm_ppp_kernel(GemmArgs g) {
    constexpr int BM = 256, BN = 256, BK = 64;
    constexpr int A_BYTES = BM * BK * 2, STAGE = (BM + BN) * BK * 2;
    constexpr int GROUP_M = 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tiles_m = (g.M + BM - 1) / BM, tiles_n = g.N / BN;
    const int ntiles = tiles_m * tiles_n;
    const int nk = g.K / BK;                                 // >= 2 (checked by the launcher)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wn = wave & 3;
    const int lrow = lane >> 3;
    const int lchunk = (lane & 7) ^ lrow;
    const int li = lane & 15, lq = lane >> 4;

    // logical tile index -> (m0, n0): XCD-first remap (L & 7 is the XCD for every tile of this workgroup
    // because gridDim.x is a multiple of 8 or equals ntiles), then GROUP_M swizzle.
    auto tile_origin = [&](int L, int& m0, int& n0) {
        const int xcd = L & 7, q = ntiles >> 3, r = ntiles & 7;
        const int pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (L >> 3);
        const int in_group = GROUP_M * tiles_n;
        const int first_m = (pid / in_group) * GROUP_M;
        const int gsz = min(tiles_m - first_m, GROUP_M);
        m0 = (first_m + (pid % in_group) % gsz) * BM;
        n0 = ((pid % in_group) / gsz) * BN;
    };

    // ---- DMA pieces of this wave (see gemm_pp_kernel): kinds 0/3 = A quarters, 1/2 = B half parts ----
    int dst[4][2];
    unsigned b_voff[2][2];                                   // tile independent
    int a_row[2][2];                                         // row inside the tile
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int piece = wn * 2 + j;
#pragma unroll
        for (int qa = 0; qa < 2; ++qa) {
            a_row[qa][j] = grp * 128 + qa * 64 + piece * 8 + lrow;
            dst[qa ? 3 : 0][j] = (grp * 128 + qa * 64 + piece * 8) * 128;
        }
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            const int chunk = grp * 2 + (piece >> 2), sub = piece & 3;
            const int rho = chunk * 64 + hb * 32 + sub * 8 + lrow;
            const int nl = rho & 15;
            const int nphys = (rho & ~31) + 8 * (nl >> 2) + 4 * ((rho >> 4) & 1) + (nl & 3);
            b_voff[hb][j] = (unsigned)nphys * (unsigned)g.K * 2u + lchunk * 16;
            dst[1 + hb][j] = A_BYTES + (chunk * 64 + hb * 32 + sub * 8) * 128;
        }
    }
    struct TileSrc { unsigned a_voff[2][2]; size_t b_base; int m0, n0; };
    auto make_src = [&](int L, TileSrc& ts) {
        tile_origin(L, ts.m0, ts.n0);
#pragma unroll
        for (int qa = 0; qa < 2; ++qa)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                ts.a_voff[qa][j] = (unsigned)min(ts.m0 + a_row[qa][j], g.M - 1) * (unsigned)g.lda * 2u + lchunk * 16;
        ts.b_base = (size_t)ts.n0 * g.K * 2;
    };
    // 2 pieces of `kind` for k-tile kt of tile `ts`, into stage buffer `buf`
    auto issue = [&](const TileSrc& ts, int kind, int kt, int buf) {
        char* base = smem + buf * STAGE;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const char* src = (kind == 0 || kind == 3)
                                  ? g.A + (size_t)ts.a_voff[kind == 3][j] + (size_t)kt * (BK * 2)
                                  : g.B + ts.b_base + (size_t)b_voff[kind - 1][j] + (size_t)kt * (BK * 2);
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src), LDS_PTR(base + dst[kind][j]), 16, 0, 0);
        }
    };

    int a_off[2], b_off[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int sw = ((ks * 4 + lq) ^ (lane & 7)) << 4;
        a_off[ks] = (grp * 128 + li) * 128 + sw;
        b_off[ks] = A_BYTES + (wn * 64 + li) * 128 + sw;
    }

    TileSrc cur, nxt;
    int L = blockIdx.x;
    make_src(L, cur);
    // prologue of the first tile: all of k-tile 0 and the k-tile-1 pieces of kinds 0..2
    issue(cur, 0, 0, 0); issue(cur, 1, 0, 0); issue(cur, 2, 0, 0); issue(cur, 3, 0, 0);
    issue(cur, 0, 1, 1); issue(cur, 1, 1, 1); issue(cur, 2, 1, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    int gk = 0;                                              // global k-tile counter of tile start (buffer parity)
    u32x4 af[4][2], bf[2][2][2];
    while (true) {
        const int Ln = L + gridDim.x;
        const bool has_next = Ln < ntiles;
        if (has_next) make_src(Ln, nxt);
        f32x4 acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        PP_BARRIER();                                        // k-tiles 0/1 of this tile visible to all waves
        if (grp == 1) PP_BARRIER();                          // group 1 runs one slot behind
        for (int t = 0; t < nk; ++t) {
            const char* sb = smem + ((gk + t) & 1) * STAGE;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int mh = (p >> 1), nh = (p == 1 || p == 2) ? 1 : 0;
                if (p == 0) {
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks)
                            bf[0][nj][ks] = *reinterpret_cast<const u32x4*>(sb + b_off[ks] + (nj * 16) * 128);
                }
                if (p == 0 || p == 2) {
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks)
                            af[mi][ks] = *reinterpret_cast<const u32x4*>(sb + a_off[ks] + (mh * 64 + mi * 16) * 128);
                }
                if (p == 1) {
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks)
                            bf[1][nj][ks] = *reinterpret_cast<const u32x4*>(sb + b_off[ks] + (32 + nj * 16) * 128);
                }
                {
                    const int kind = (p == 0) ? 3 : p - 1;
                    const int itile = (p == 0) ? t + 1 : t + 2;
                    const int buf = (gk + itile) & 1;
                    bool issued = true;
                    if (itile < nk) issue(cur, kind, itile, buf);
                    else if (has_next) issue(nxt, kind, itile - nk, buf);
                    else issued = false;
                    if (!issued) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    else if (t > 0) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                    // t == 0: every k-tile-0/1 piece this tile reads before k-tile 1 was drained before the
                    // previous epilogue (or in the prologue); stores may still be in flight -> no counted wait.
                }
                PP_BARRIER();
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                        for (int nj = 0; nj < 2; ++nj)
                            acc[mh * 4 + mi][nh * 2 + nj] = T::mfma16(bf[nh][nj][ks], af[mi][ks], acc[mh * 4 + mi][nh * 2 + nj]);
                __builtin_amdgcn_s_setprio(0);
                PP_BARRIER();
            }
        }
        if (grp == 0) PP_BARRIER();                          // balance group 1's extra barrier
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's DMA for the next tile has landed
        if (cur.m0 + BM <= g.M) epilogue_wave<T, EPI, 8, 4, true>(g, acc, cur.m0 + grp * 128 + (lane & 15), cur.n0 + wn * 64 + 8 * (lane >> 4));
        else epilogue_wave<T, EPI, 8, 4, false>(g, acc, cur.m0 + grp * 128 + (lane & 15), cur.n0 + wn * 64 + 8 * (lane >> 4));   // (no LayerNorm fold in this variant)
        if (!has_next) break;
        cur = nxt;
        L = Ln;
        gk += nk;
    }
}

template <typename T, int EPI, int KTAG>
static int launch_ppp_k(const GemmArgs& g, hipStream_t stream) {
    constexpr int LDS = 2 * (256 + 256) * 64 * 2;
    auto kern = gemm_ppp_kernel<T, EPI, KTAG>;
    SLIME_SET_LDS_ONCE(kern, LDS, "gemm_ppp");
    const int g_num_cu = num_cus();
    const int ntiles = ((g.M + 255) / 256) * (g.N / 256);
    int grid = ntiles < g_num_cu ? ntiles : (g_num_cu / 8) * 8;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), LDS, stream, g);
    SLIME_CHECK_LAUNCH("gemm_ppp");
    return SLIME_OK;
}
template <typename T, int EPI>
static int launch_ppp(const GemmArgs& g, hipStream_t stream) {
    return g.K >= 2048 ? launch_ppp_k<T, EPI, 1>(g, stream) : launch_ppp_k<T, EPI, 0>(g, stream);
}


// ================================================================================================
// 32x32x16 MFMA variant (measured alternative, not the default): 1024 vs ~915 flop/cycle/SIMD of issue
// bound, half the matrix instructions and operand reads per flop.  A first version with the 4-phase table
// of gemm_pp_kernel (8 MFMAs on 2 accumulators per M section) was bound by the 64-cycle dependent latency
// (-15 %); the 2-phase kernel below removes that and still trails the 16x16 kernel by ~10 % (1075 vs
// 1230 TF/s at K = 4096): its L sections (16 fragment reads drained before the barrier) are long.
//   * fragments: a lane feeds row (lane & 31), k = 8*(lane >> 5) .. +7 of a 16-deep k-step
//     -> ds_read_b128 of chunk 2*ks + (lane >> 5); the 16-lane ds_read_b128 groups then touch 16
//     different rows with one chunk index, so the swizzle key is (row >> 1) & 7 (8 distinct keys per row
//     parity inside every group) instead of row & 7;
//   * D layout: col = lane & 31 (the X row m), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (the W row n);
//     W rows are permuted inside each 32-row tile while staging so that D row index i maps to
//     n = 16*(lane>>5) + r: a lane owns 16 consecutive output columns of one row.
// ================================================================================================
template <typename T, int EPI, bool FULL>
__device__ __forceinline__ void epilogue_wave32(const GemmArgs& g, f32x16 (&acc)[4][2], const int row_base, const int col_base) {
    // row_base: m0 + grp*128 + (lane & 31); col_base: n0 + wn*64 + 16*(lane >> 5); tile (mi, nj) adds (32 mi, 32 nj)
    float bias[2][16];
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
        for (int v4 = 0; v4 < 4; ++v4) {
            float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g.bias) bv = *reinterpret_cast<const float4*>(g.bias + col_base + 32 * nj + 4 * v4);
            bias[nj][4 * v4 + 0] = bv.x; bias[nj][4 * v4 + 1] = bv.y; bias[nj][4 * v4 + 2] = bv.z; bias[nj][4 * v4 + 3] = bv.w;
        }
    auto in_range = [&](int row) { return FULL || row < g.M; };
    if constexpr (EPI == SLIME_EPI_BIAS_RESID_F32) {
        float* C = reinterpret_cast<float*>(g.C);
        float4 hb[2][2][4];                                   // [buffer][nj][v4]: one 32-row step ahead
        auto load_step = [&](int mi, int buf) {
            int row = row_base + mi * 32;
            if constexpr (!FULL) row = min(row, g.M - 1);
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int v4 = 0; v4 < 4; ++v4)
                    hb[buf][nj][v4] = *reinterpret_cast<const float4*>(C + (size_t)row * g.ldc + col_base + 32 * nj + 4 * v4);
        };
        load_step(0, 0);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            if (mi + 1 < 4) load_step(mi + 1, (mi + 1) & 1);
            const int row = row_base + mi * 32;
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
#pragma unroll
                for (int v4 = 0; v4 < 4; ++v4) {
                    const float4 hv = hb[mi & 1][nj][v4];
                    acc[mi][nj][4 * v4 + 0] += bias[nj][4 * v4 + 0] + hv.x; acc[mi][nj][4 * v4 + 1] += bias[nj][4 * v4 + 1] + hv.y;
                    acc[mi][nj][4 * v4 + 2] += bias[nj][4 * v4 + 2] + hv.z; acc[mi][nj][4 * v4 + 3] += bias[nj][4 * v4 + 3] + hv.w;
                }
                if (in_range(row)) {
                    float* o = C + (size_t)row * g.ldc + col_base + 32 * nj;
#pragma unroll
                    for (int v4 = 0; v4 < 4; ++v4)
                        *reinterpret_cast<float4*>(o + 4 * v4) = make_float4(acc[mi][nj][4 * v4], acc[mi][nj][4 * v4 + 1], acc[mi][nj][4 * v4 + 2], acc[mi][nj][4 * v4 + 3]);
                }
            }
        }
    } else {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float a = acc[mi][nj][r] + bias[nj][r];
                    if constexpr (EPI == SLIME_EPI_BIAS_QUICKGELU_T) a = a * __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * a));
                    else if constexpr (EPI == SLIME_EPI_BIAS_GELU_T) a = gelu_erf(a);
                    else if constexpr (EPI == SLIME_EPI_BIAS_GELU_TANH_T) a = gelu_tanh(a);
                    acc[mi][nj][r] = a;
                }
        if constexpr (EpiOutIsT<EPI>::value) {
            u32x4 packed[4][2][2];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                    for (int hv = 0; hv < 2; ++hv)
#pragma unroll
                        for (int w = 0; w < 4; ++w) packed[mi][nj][hv][w] = T::pack2(acc[mi][nj][8 * hv + 2 * w], acc[mi][nj][8 * hv + 2 * w + 1]);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int row = row_base + mi * 32;
                if (in_range(row)) {
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj) {
                        char* o = reinterpret_cast<char*>(g.C) + ((size_t)row * g.ldc + col_base + 32 * nj) * 2;
                        *reinterpret_cast<u32x4*>(o) = packed[mi][nj][0];
                        *reinterpret_cast<u32x4*>(o + 16) = packed[mi][nj][1];
                    }
                }
            }
        } else {
            float* C = reinterpret_cast<float*>(g.C);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int row = row_base + mi * 32;
                if (in_range(row)) {
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj) {
                        float* o = C + (size_t)row * g.ldc + col_base + 32 * nj;
#pragma unroll
                        for (int v4 = 0; v4 < 4; ++v4)
                            *reinterpret_cast<float4*>(o + 4 * v4) = make_float4(acc[mi][nj][4 * v4], acc[mi][nj][4 * v4 + 1], acc[mi][nj][4 * v4 + 2], acc[mi][nj][4 * v4 + 3]);
                    }
                }
            }
        }
    }
}

// ================================================================================================
// gemm_pp32b_kernel: 32x32x16 MFMA, TWO phases per k-tile.
// The 4-phase 32x32 kernel above accumulates 8 MFMAs on 2 accumulators per M section and is bound by the
// 64-cycle dependent latency of v_mfma_f32_32x32x16 (measured 15 % slower than the 16x16 kernel).  Here a
// phase is a 64x64 half of the wave tile: 4 independent accumulators x 4 k-steps = 16 MFMAs (~512 cycles),
// so the matrix pipe streams at its issue rate and there are half as many barriers per k-tile.
//
// Slots: tile t phase p -- group 0: L at 4t+2p, M at 4t+2p+1; group 1 one slot later.  Every L section
// ends with lgkmcnt(0) BEFORE its barrier, so a region is free for refill one slot after its last reader's
// L section.  Readers: A(own half, rows 0..63) and all of B in L0, A(rows 64..127) in L1.  Refill of the
// stage buffer for tile t+2 (4 pieces per wave per section):
//     L1(t)   : this group's half of the B tile of t+2      (B last read by group 1 in slot 4t+1)
//     L0(t+1) : this group's 128 A rows of t+2              (last read in L1(t), slots 4t+2 / 4t+3)
// and every L1 section retires all but its own 4 newest pieces (vmcnt(4)) one barrier or more before
// their first reader (L0(t+2)); a piece is in flight for >= 2 slots (~1100 cycles).
// ================================================================================================
template <typename T, int EPI, int KTAG>
__global__ void __launch_bounds__(512) gemm_pp32b_kernel(GemmArgs g) {
    constexpr int BM = 256, BN = 256, BK = 64;
    constexpr int A_BYTES = BM * BK * 2, STAGE = (BM + BN) * BK * 2;
    constexpr int GROUP_M = 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tiles_m = (g.M + BM - 1) / BM, tiles_n = g.N / BN;
    const int nblk = tiles_m * tiles_n;
    int pid;
    {
        const int b = blockIdx.x, xcd = b & 7, q = nblk >> 3, r = nblk & 7;
        pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
    }
    const int in_group = GROUP_M * tiles_n;
    const int first_m = (pid / in_group) * GROUP_M;
    const int gsz = min(tiles_m - first_m, GROUP_M);
    const int tm = first_m + (pid % in_group) % gsz;
    const int tn = (pid % in_group) / gsz;
    const int m0 = tm * BM, n0 = tn * BN;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wn = wave & 3;
    const int lrow = lane >> 3, cpos = lane & 7;
    const int l31 = lane & 31, lh = lane >> 5;

    // ---- LDS-DMA pieces: kind 0 = 4 pieces of this group's A half (16 pieces, 4 per wave),
    //                      kind 1 = 4 pieces of this group's half of the B tile (rows grp*128 .. +127) ----
    const char* src[2][4];
    int dst[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int piece = wn * 4 + j;                                   // 0..15: 8-row piece inside the 128-row half
        {
            const int row = grp * 128 + piece * 8;
            const int key = ((row + lrow) >> 1) & 7;
            const int gm = min(m0 + row + lrow, g.M - 1);
            src[0][j] = g.A + ((size_t)gm * g.lda) * 2 + ((cpos ^ key) << 4);
            dst[0][j] = row * 128;
        }
        {
            const int rho = grp * 128 + piece * 8 + lrow;               // LDS row of the B tile
            const int key = (rho >> 1) & 7;
            const int r32 = rho & 31;
            const int nphys = (rho & ~31) + 16 * ((r32 >> 2) & 1) + 4 * (r32 >> 3) + (r32 & 3);
            src[1][j] = g.B + ((size_t)(n0 + nphys) * g.K) * 2 + ((cpos ^ key) << 4);
            dst[1][j] = A_BYTES + (grp * 128 + piece * 8) * 128;
        }
    }
    auto issue = [&](int kind, int tile) {
        char* base = smem + (tile & 1) * STAGE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src[kind][j]), LDS_PTR(base + dst[kind][j]), 16, 0, 0);
            src[kind][j] += BK * 2;
        }
    };

    int a_off[4], b_off[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const int sw = ((ks * 2 + lh) ^ ((lane >> 1) & 7)) << 4;
        a_off[ks] = (grp * 128 + l31) * 128 + sw;
        b_off[ks] = A_BYTES + (wn * 64 + l31) * 128 + sw;
    }

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = g.K / BK;
    issue(0, 0); issue(1, 0);                                 // all of tile 0
    if (nk > 1) {
        issue(1, 1);                                          // B of tile 1 (an "L1(-1)" piece set); A(1) comes in L0(0)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    PP_BARRIER();
    if (grp == 1) PP_BARRIER();

    u32x4 af[2][4], bf[2][4];
    for (int t = 0; t < nk; ++t) {
        const char* sb = smem + (t & 1) * STAGE;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            // ---------------- L section ----------------
            if (p == 0) {
#pragma unroll
                for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) bf[nj][ks] = *reinterpret_cast<const u32x4*>(sb + b_off[ks] + nj * 32 * 128);
            }
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    af[mi][ks] = *reinterpret_cast<const u32x4*>(sb + a_off[ks] + (p * 64 + mi * 32) * 128);
            if (p == 0) {                                     // L0(t): this group's A rows of tile t+1
                if (t + 1 < nk) issue(0, t + 1);
            } else {                                          // L1(t): this group's B half of tile t+2; retire the rest
                if (t + 2 < nk) { issue(1, t + 2); asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            // the fragment reads must have LEFT the LDS before the other group may refill what they read
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[0][0]), "+v"(af[0][1]), "+v"(af[0][2]), "+v"(af[0][3]),
                                                   "+v"(af[1][0]), "+v"(af[1][1]), "+v"(af[1][2]), "+v"(af[1][3]));
            if (p == 0)
                asm volatile("" : "+v"(bf[0][0]), "+v"(bf[0][1]), "+v"(bf[0][2]), "+v"(bf[0][3]),
                                  "+v"(bf[1][0]), "+v"(bf[1][1]), "+v"(bf[1][2]), "+v"(bf[1][3]));
            PP_BARRIER();
            // ---------------- M section: 64 x 64 half, 4 accumulators x 4 k-steps ----------------
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
                        acc[p * 2 + mi][nj] = T::mfma32(bf[nj][ks], af[mi][ks], acc[p * 2 + mi][nj]);
            __builtin_amdgcn_s_setprio(0);
            PP_BARRIER();
        }
    }
    if (grp == 0) PP_BARRIER();

    if (m0 + BM <= g.M) epilogue_wave32<T, EPI, true>(g, acc, m0 + grp * 128 + l31, n0 + wn * 64 + 16 * lh);
    else epilogue_wave32<T, EPI, false>(g, acc, m0 + grp * 128 + l31, n0 + wn * 64 + 16 * lh);
}

template <typename T, int EPI, int KTAG>
static int launch_pp32b_k(const GemmArgs& g, hipStream_t stream) {
    constexpr int LDS = 2 * (256 + 256) * 64 * 2;
    auto kern = gemm_pp32b_kernel<T, EPI, KTAG>;
    SLIME_SET_LDS_ONCE(kern, LDS, "gemm_pp32b");
    const int tiles_m = (g.M + 255) / 256, tiles_n = g.N / 256;
    hipLaunchKernelGGL(kern, dim3(tiles_m * tiles_n), dim3(512), LDS, stream, g);
    SLIME_CHECK_LAUNCH("gemm_pp32b");
    return SLIME_OK;
}
template <typename T, int EPI>
static int launch_pp32b(const GemmArgs& g, hipStream_t stream) {
    return g.K >= 2048 ? launch_pp32b_k<T, EPI, 1>(g, stream) : launch_pp32b_k<T, EPI, 0>(g, stream);
}

// Round 4's persistent direct-B kernels with the epilogue in the next tile's MFMA stream (gemm_ps.hip: gemm_ps32.inc, gemm_ps.inc):
// bit-identical to the kernels here, measured SLOWER than gemm_db_kernel (profiles/r04_ps_ablation.txt) -- measured alternatives,
// tiles 16 / 17, in their own translation unit of the diagnostic library.
bool slime_diag_ps_usable(const GemmArgs& g, int epi);
int slime_diag_launch_ps(const GemmArgs& g, int dtype, int epi, int tile, hipStream_t stream);

// 192 x 256 ping-pong tiles (tile 9): measured alternative for the sub-round grids, see auto_tile
template <typename T, int EPI>
static int launch_pp192(const GemmArgs& g, hipStream_t stream) {
    return g.K >= 2048 ? launch_pp_k<T, EPI, 1, 0, 3>(g, stream) : launch_pp_k<T, EPI, 0, 0, 3>(g, stream);
}

// Timing ablations of gemm_pp_kernel / gemm_w4_kernel (the ABL template parameter, slime_gemm_set_ablation), tried in front of launch_pp /
// launch_w4 <.., 8>.
template <typename T, int EPI>
static std::optional<int> launch_pp_ablation(const GemmArgs& g, hipStream_t stream) {
    if constexpr (EPI == SLIME_EPI_BIAS_T && T::id == SLIME_BF16) {     // ablation builds: one epilogue only
        switch (g_ablation) {
            case 1: return launch_pp_k<T, EPI, 0, 1>(g, stream);
            case 2: return launch_pp_k<T, EPI, 0, 2>(g, stream);
            case 3: return launch_pp_k<T, EPI, 0, 3>(g, stream);
            case 4: return launch_pp_k<T, EPI, 0, 4>(g, stream);
            case 7: return launch_pp_k<T, EPI, 0, 7>(g, stream);
            case 8: return launch_pp_k<T, EPI, 0, 8>(g, stream);
            default: break;
        }
    }
    return std::nullopt;
}
template <typename T, int EPI, int MI>
static std::optional<int> launch_w4_ablation(const GemmArgs& g, hipStream_t stream) {
    if constexpr (EPI == SLIME_EPI_BIAS_T && T::id == SLIME_BF16 && MI == 8) {     // ablation builds: one configuration only
        switch (g_ablation) {
            case 1: return launch_w4_k<T, EPI, 0, MI, 1>(g, stream);
            case 2: return launch_w4_k<T, EPI, 0, MI, 2>(g, stream);
            case 3: return launch_w4_k<T, EPI, 0, MI, 3>(g, stream);
            case 4: return launch_w4_k<T, EPI, 0, MI, 4>(g, stream);
            case 7: return launch_w4_k<T, EPI, 0, MI, 7>(g, stream);
            case 8: return launch_w4_k<T, EPI, 0, MI, 8>(g, stream);   // split barrier on an LDS counter (correct results)
            default: break;
        }
    }
    return std::nullopt;
}

// The diagnostic part of launch_epi, called with auto_tile's choice: the forced tile or the per-shape rule replaces it, tiles the
// shape or the epilogue cannot run are rewritten, and the kernels only this build has are launched from here (the launch status is
// returned).  Without a value, launch_epi goes on with `tile` through the branches both builds share.
template <typename T, int EPI>
static std::optional<int> diag_launch_epi(const GemmArgs& g, hipStream_t stream, int& tile) {
    if (g_force_tile != 0) tile = g_force_tile;
    else
        for (int i = 0; i < g_rules; ++i)
            if (g_rule_n[i] == g.N && g_rule_k[i] == g.K) tile = g_rule_tile[i];
    if (tile == 2) tile = 1;
    if ((!g.B || g.row_map) && (tile == 5 || tile == 6 || tile == 7 || tile == 8)) tile = 4;   // persistent / 32x32 ping-pong variants: row-major B only, no row map
    if ((tile == 1 || (tile >= 4 && tile != 15 && tile != 18)) && g.N % 256 != 0) tile = 3;
    if ((tile == 12 || tile == 13 || tile == 19) && !g.Bf) tile = tile == 13 ? 3 : 11;
    if (tile == 6 || tile == 8) tile = 7;
    if (tile == 7 && (EPI == SLIME_EPI_BIAS_RESID_F32_LN || EPI == SLIME_EPI_BIAS_RESID_T || EPI == SLIME_EPI_BIAS_RESID_SPLIT_LN)) tile = 4;     // the 32x32 variant has neither epilogue
    if (tile == 7) return launch_pp32b<T, EPI>(g, stream);
    if (tile == 5 && g.K < 128) tile = 4;                              // persistent kernel needs >= 2 k-tiles
    if (tile == 5 && ((size_t)g.M * g.lda * 2 >= (1ull << 32) || (size_t)g.N * g.K * 2 >= (1ull << 32))) tile = 4;   // 32-bit row offsets
    if (tile == 5) return launch_ppp<T, EPI>(g, stream);
    if (tile == 9) return launch_pp192<T, EPI>(g, stream);
    if (tile == 1) return g_sched == 0 ? launch_cfg<T, 256, 256, 2, 4, EPI, 0>(g, stream) : launch_cfg<T, 256, 256, 2, 4, EPI, 1>(g, stream);
    if (tile == 3 && g_sched == 0) return launch_cfg<T, 128, 128, 2, 2, EPI, 0>(g, stream);
    if (tile == 16 || tile == 17) {                                        // persistent direct-B, measured alternatives: 16 = 16x16x32 MFMAs, 17 = 32x32x16
        if (slime_diag_ps_usable(g, EPI)) return slime_diag_launch_ps(g, T::id, EPI, tile, stream);
        tile = g.Bf ? 12 : 11;
    }
    if (tile == 19) {                                             // measured alternative (96-row direct-B tiles), see auto_tile
        if constexpr (db96_epilogue(EPI)) {
            if (g.Bf) return launch_db<T, EPI, 6>(g, stream);
        }
        return launch_db<T, EPI, 8>(g, stream);
    }
    if (tile == 13) return launch_db<T, EPI, 4>(g, stream);       // measured alternative (64-row direct-B tiles), see gemm_db_kernel
    // the ablation builds stand in for the kernel launch_epi would launch from here: its B = NULL rule decides which one that is
    const int last = (!g.B && (tile == 10 || tile == 11)) ? (g.Bf ? 12 : 4) : tile;
    if (last == 4) return launch_pp_ablation<T, EPI>(g, stream);
    if (last == 11) return launch_w4_ablation<T, EPI, 8>(g, stream);
    return std::nullopt;
}

// The GemmArgs fields that come from hooks (literal zeros in the product build).
static void diag_hook_args(GemmArgs& g) { g.group_m = g_group_m; g.dbg = g_dbg; g.db_abl = g_db_abl; }
