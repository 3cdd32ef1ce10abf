// gemm_ksplit.inc -- included by gemm.hip: the opt-in DETERMINISTIC split-K form of the LDS-staged GEMM (slime_gemm_ksplit).
//
// A tower pass over 1-9 crops launches sub-round grids (fc2 at 5 crops: 184 workgroups of 128 x 128 x 4096 on 256 CUs; at one crop
// every GEMM of a layer), and each workgroup walks a dependent chain of 16-64 k-tiles alone.  Splitting K gives the idle CUs work.
// The split is an ARGUMENT, never derived from the grid: workgroup (tile, s) of the partial kernel multiplies the k-tiles
//     [floor(s nk / S), floor((s + 1) nk / S))       nk = K / 64, S = splits
// from zero accumulators, in the k order of gemm_kernel, and stores its accumulators as they are; the reduce kernel sums the S
// planes in the fixed order ((p0 + p1) + p2) + ... in fp32 and runs the SAME run_epilogue on the sum.  So an output element is a
// function of its row of A, of B and of (K, S) alone -- not of M, of the tile, or of how the rows are cut into calls or rank shards.
// What is given up is bit-equality between two different S.
//
// The two launches are ordered by the stream alone: no atomics, no flags, no waiting between workgroups.
//
// Partial planes (internal to the pair of launches): f32x4 [s][tile = tm * tiles_n + tn][wave][i][j][lane] -- one 16-byte store per
// lane and fragment, 1 KiB contiguous per wave; a tile is BM * BN * 4 bytes, a plane tiles_m * BM * N * 4.  Offsets are 32-bit
// (slime_gemm_ksplit refuses a partial buffer of 4 GiB or more).

// Main loop = gemm_kernel's three-stage ring (SCHED == 2), restated here because gemm_kernel's symbol names are part of what the
// benchmark reports (slime_gemm_kernel_name) and its code is not to move: k-tile t of the chunk lives in stage t % 3, its DMA is
// issued two tiles ahead, and the counted wait leaves the next tile's pieces in flight.  A chunk of 1 or 2 k-tiles is covered by
// the same guards as nk = 1 / 2 there (the second prologue stage and the look-ahead are conditional; the last tile drains to 0).
template <typename T, int BM, int BN, int WAVES_M, int WAVES_N>
__global__ void __launch_bounds__(WAVES_M * WAVES_N * 64)
gemm_ksplit_partial_kernel(GemmArgs g, char* __restrict__ ws, const int splits) {
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int TM = BM / WAVES_M, TN = BN / WAVES_N;
    constexpr int MI = TM / 16, NI = TN / 16;
    constexpr int BK = 64;
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int A_INSTR = BM / 8 / NW, B_INSTR = BN / 8 / NW;
    static_assert(NI % 2 == 0 && A_INSTR >= 1 && B_INSTR >= 1, "tile shape");
    static_assert(A_INSTR + B_INSTR == 8 || A_INSTR + B_INSTR == 4, "counted wait below: 8 (128 x 128) or 4 (64 x 64) pieces per wave and stage");
    constexpr int GROUP_M = 8;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    // ---- (tile, split) of this workgroup: XCD-first remap over the whole grid, splits outermost, GROUP_M swizzle inside a split
    const int tiles_m = (g.M + BM - 1) / BM, tiles_n = g.N / BN;
    const int ntiles = tiles_m * tiles_n, nblk = ntiles * splits;
    int pid;
    {
        const int b = blockIdx.x, xcd = b & 7, q = nblk >> 3, r = nblk & 7;
        pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
    }
    const int split = pid / ntiles;
    pid -= split * ntiles;
    const int in_group = GROUP_M * tiles_n;
    const int group_id = pid / in_group;
    const int first_m = group_id * GROUP_M;
    const int gsz = min(tiles_m - first_m, GROUP_M);
    const int tm = first_m + (pid % in_group) % gsz;
    const int tn = (pid % in_group) / gsz;
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- this split's k-tiles: a function of (K, splits) alone
    const int nk_all = g.K / BK;
    const int k0 = (int)((long)split * nk_all / splits), k1 = (int)((long)(split + 1) * nk_all / splits);
    const int nk = k1 - k0;                               // >= 1: splits <= K / 64 (checked by slime_gemm_ksplit)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int lrow = lane >> 3;                       // row inside the 8-row piece == (LDS row & 7)
    const int lchunk = (lane & 7) ^ lrow;             // swizzled 16-B chunk of the 128-B k-slab

    // the static operand: row-major image (k-tile advance 128 bytes) or, with B == NULL, the fragment-order image (8 KiB)
    const bool bfrag = g.B == nullptr;
    const int b_kstep = bfrag ? (int)FRAG_KTILE_BYTES : BK * 2;
    const char* b_tile0 = (bfrag ? g.Bimg : g.B) + (size_t)n0 * g.K * 2;

    int a_off[2], b_off[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int sw = ((ks * 4 + (lane >> 4)) ^ (lane & 7)) << 4;
        a_off[ks] = (wm * TM + (lane & 15)) * 128 + sw;
        b_off[ks] = bfrag ? A_BYTES + wn * TN * 128 + ks * 1024 + lane * 16 : A_BYTES + (wn * TN + (lane & 15)) * 128 + sw;
    }

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    unsigned soff[A_INSTR + B_INSTR];
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i) {
        const int r = (i * NW + wave) * 8 + lrow;
        soff[i] = (unsigned)min(r, g.M - 1 - m0) * (unsigned)g.lda * 2u + lchunk * 16;     // clamp: rows past M re-read the last row
    }
#pragma unroll
    for (int i = 0; i < B_INSTR; ++i) {
        const int rho = (i * NW + wave) * 8 + lrow, nl = rho & 15;
        const int nphys = (rho & ~31) + 8 * (nl >> 2) + 4 * ((rho >> 4) & 1) + (nl & 3);
        const int q = i * NW + wave;
        soff[A_INSTR + i] = bfrag ? frag_piece_offset(q >> 1, q & 1, g.K) + lane * 16 : (unsigned)nphys * (unsigned)g.K * 2u + lchunk * 16;
    }
    const char* a_gbase = g.A + (size_t)m0 * g.lda * 2 + (size_t)k0 * (BK * 2);
    const char* b_gbase = b_tile0 + (size_t)k0 * b_kstep;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_byte_addr(smem));
    auto stage3 = [&](int tile) {                         // tile: k-tile counted from the chunk's first
        const unsigned base = lds0 + (tile % 3) * STAGE;
        const char* ga = uniform_ptr(a_gbase + (size_t)tile * (BK * 2));
        const char* gb = uniform_ptr(b_gbase + (size_t)tile * b_kstep);
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) lds_dma16(soff[i], ga, base + (i * NW + wave) * 1024);
#pragma unroll
        for (int i = 0; i < B_INSTR; ++i) lds_dma16(soff[A_INSTR + i], gb, base + A_BYTES + (i * NW + wave) * 1024);
    };
    stage3(0);
    if (nk > 1) stage3(1);
    for (int kt = 0; kt < nk; ++kt) {
        // k-tile kt has landed (its pieces are older than those of k-tile kt+1); every wave has finished reading k-tile kt-1
        if (kt + 1 < nk) {
            if constexpr (A_INSTR + B_INSTR == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 2 < nk) stage3(kt + 2);                  // into the stage k-tile kt-1 was read from
        const char* sb = smem + (kt % 3) * STAGE;
        u32x4 bf0[NI], af0[MI], bf1[NI], af1[MI];
#pragma unroll
        for (int j = 0; j < NI; ++j) bf0[j] = *reinterpret_cast<const u32x4*>(sb + b_off[0] + j * 2048);
#pragma unroll
        for (int i = 0; i < MI; ++i) af0[i] = *reinterpret_cast<const u32x4*>(sb + a_off[0] + i * 2048);
#pragma unroll
        for (int j = 0; j < NI; ++j) bf1[j] = *reinterpret_cast<const u32x4*>(sb + b_off[1] + j * 2048);
#pragma unroll
        for (int i = 0; i < MI; ++i) af1[i] = *reinterpret_cast<const u32x4*>(sb + a_off[1] + i * 2048);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = T::mfma16(bf0[j], af0[i], acc[i][j]);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = T::mfma16(bf1[j], af1[i], acc[i][j]);
        if constexpr (MI * NI >= MI + NI) {
            __builtin_amdgcn_sched_group_barrier(0x100, MI + NI, 0);
#pragma unroll
            for (int r = 0; r < MI + NI; ++r) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * MI * NI - 2 * (MI + NI), 0);
        }
    }

    // ---- no epilogue: the accumulators as they are, fragment order (rows past M included: the reduce kernel's row guard drops them)
    char* dst = ws + (unsigned)(split * ntiles + tm * tiles_n + tn) * (unsigned)(BM * BN * 4) + (unsigned)(wave * MI * NI) * 1024u + lane * 16;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) *reinterpret_cast<f32x4*>(dst + (i * NI + j) * 1024) = acc[i][j];
}

// One workgroup per output tile, the wave / lane <-> element mapping of the partial kernel (= gemm_kernel's): a lane sums its
// fragments of the S planes in plane order and hands them to run_epilogue -- the epilogue code of every other kernel in gemm.hip.
template <typename T, int BM, int BN, int WAVES_M, int WAVES_N, int EPI>
__global__ void __launch_bounds__(WAVES_M * WAVES_N * 64)
gemm_ksplit_reduce_kernel(GemmArgs g, const char* __restrict__ ws, const int splits) {
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int TM = BM / WAVES_M, TN = BN / WAVES_N;
    constexpr int MI = TM / 16, NI = TN / 16;
    __shared__ __attribute__((aligned(16))) float lnrow[2 * BM];

    const int tiles_m = (g.M + BM - 1) / BM, tiles_n = g.N / BN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;      // consecutive workgroups: the column tiles of one row tile
    const int m0 = tm * BM, n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;

    stage_ln_rows<BM, NW * 64>(g, m0, lnrow);             // (rstd, -mu rstd) of the tile's rows when the call folds a LayerNorm

    const unsigned plane = (unsigned)(tiles_m * tiles_n) * (unsigned)(BM * BN * 4);
    const char* src = ws + (unsigned)blockIdx.x * (unsigned)(BM * BN * 4) + (unsigned)(wave * MI * NI) * 1024u + lane * 16;
    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = *reinterpret_cast<const f32x4*>(src + (i * NI + j) * 1024);
    for (int s = 1; s < splits; ++s) {                    // ((p0 + p1) + p2) + ...: plane order, one fp32 add per element and plane
        src += plane;
        f32x4 p[MI][NI];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) p[i][j] = *reinterpret_cast<const f32x4*>(src + (i * NI + j) * 1024);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = acc[i][j] + p[i][j];
    }
    __syncthreads();                                      // publishes the row table to the other waves
    run_epilogue<T, EPI, MI, NI>(g, acc, m0 + wm * TM + (lane & 15), n0 + wn * TN + 8 * (lane >> 4), m0 + BM <= g.M,
                                 lnrow + 2 * (wm * TM + (lane & 15)));
}

template <typename T, int BM, int BN, int WAVES_M, int WAVES_N>
static int launch_ksplit_partial(const GemmArgs& g, char* ws, int splits, hipStream_t stream) {
    constexpr int LDS = 3 * (BM + BN) * 64 * 2;
    auto kern = gemm_ksplit_partial_kernel<T, BM, BN, WAVES_M, WAVES_N>;
    SLIME_SET_LDS_ONCE(kern, LDS, "gemm_ksplit");
    const int tiles_m = (g.M + BM - 1) / BM, tiles_n = g.N / BN;
    hipLaunchKernelGGL(kern, dim3(tiles_m * tiles_n * splits), dim3(WAVES_M * WAVES_N * 64), LDS, stream, g, ws, splits);
    SLIME_CHECK_LAUNCH("gemm_ksplit (partial products)");
    return SLIME_OK;
}

template <typename T, int BM, int BN, int WAVES_M, int WAVES_N, int EPI>
static int launch_ksplit_reduce(const GemmArgs& g, const char* ws, int splits, hipStream_t stream) {
    const int tiles_m = (g.M + BM - 1) / BM, tiles_n = g.N / BN;
    hipLaunchKernelGGL((gemm_ksplit_reduce_kernel<T, BM, BN, WAVES_M, WAVES_N, EPI>), dim3(tiles_m * tiles_n), dim3(WAVES_M * WAVES_N * 64),
                       0, stream, g, ws, splits);
    SLIME_CHECK_LAUNCH("gemm_ksplit (reduce + epilogue)");
    return SLIME_OK;
}

template <typename T, int BM, int BN, int WAVES_M, int WAVES_N>
static int launch_ksplit_tile(const GemmArgs& g, int epi, char* ws, int splits, hipStream_t stream) {
    if (const int rc = launch_ksplit_partial<T, BM, BN, WAVES_M, WAVES_N>(g, ws, splits, stream)) return rc;
    switch (epi) {
#define KSPLIT_EPI(E) case E: return launch_ksplit_reduce<T, BM, BN, WAVES_M, WAVES_N, E>(g, ws, splits, stream);
        KSPLIT_EPI(SLIME_EPI_BIAS_T) KSPLIT_EPI(SLIME_EPI_BIAS_QUICKGELU_T) KSPLIT_EPI(SLIME_EPI_BIAS_GELU_T) KSPLIT_EPI(SLIME_EPI_BIAS_F32)
        KSPLIT_EPI(SLIME_EPI_BIAS_RESID_F32) KSPLIT_EPI(SLIME_EPI_BIAS_RESID_F32_LN) KSPLIT_EPI(SLIME_EPI_BIAS_RESID_T)
        KSPLIT_EPI(SLIME_EPI_BIAS_RESID_SPLIT_LN) KSPLIT_EPI(SLIME_EPI_BIAS_GELU_TANH_T)
#undef KSPLIT_EPI
    }
    return SLIME_EINVAL;                                  // unreachable: slime_gemm_ksplit checked the epilogue before the first launch
}

// Tile of the pair (the same for both launches): 64 x 64 where 128 x 128 workgroups x splits would leave half the CUs idle -- the
// rule auto_tile applies to the unsplit three-stage kernel, with the split counted in.  It may depend on M and on the CU count:
// both tiles accumulate an element over the same k order and run the same epilogue, so the results are the same bits.
template <typename T>
static int launch_ksplit_T(const GemmArgs& g, int epi, char* ws, int splits, hipStream_t stream) {
    const long wg128 = (long)((g.M + 127) / 128) * (g.N / 128) * splits;
    if (wg128 * 2 <= num_cus()) return launch_ksplit_tile<T, 64, 64, 4, 1>(g, epi, ws, splits, stream);
    return launch_ksplit_tile<T, 128, 128, 2, 2>(g, epi, ws, splits, stream);
}

extern "C" size_t slime_gemm_ksplit_workspace_bytes(int M, int N, int splits) {
    if (M <= 0 || N <= 0 || splits < 2 || splits > SLIME_GEMM_KSPLIT_MAX) return 0;          // splits == 1: no partial planes
    return align_up((size_t)splits * ((size_t)(M + 127) / 128 * 128) * (size_t)N * sizeof(float), 256);   // 128-row tiles cover the 64-row form
}

extern "C" int slime_gemm_ksplit(const slime_gemm_args* a, int splits, void* ws, size_t ws_bytes, void* stream) {
    SLIME_REQUIRE(a, "gemm_ksplit: null argument block");
    SLIME_REQUIRE(splits >= 1 && splits <= SLIME_GEMM_KSPLIT_MAX, "gemm_ksplit: splits=%d outside 1..%d", splits, SLIME_GEMM_KSPLIT_MAX);
    if (splits == 1) return slime_gemm_ex(a, stream);     // the unsplit path itself: no workspace
    GemmArgs g;
    if (const int rc = gemm_check_args(a, g)) return rc;
    SLIME_REQUIRE(splits <= a->K / 64, "gemm_ksplit: splits=%d above K / 64 = %d (every split multiplies at least one 64-wide k-tile)",
                  splits, a->K / 64);
    SLIME_REQUIRE(a->epilogue != SLIME_EPI_BIAS_GELU_MIX_T, "gemm_ksplit: BIAS_GELU_MIX_T runs on the direct-B kernel only; the split is built "
                                                             "for the LDS-staged kernel");
    SLIME_REQUIRE(a->epilogue >= SLIME_EPI_BIAS_T && a->epilogue <= SLIME_EPI_BIAS_GELU_TANH_T, "gemm: unknown epilogue %d", a->epilogue);
    SLIME_REQUIRE(a->dtype == SLIME_BF16 || a->dtype == SLIME_F16, "gemm: dtype %d is not a 16-bit MFMA type", a->dtype);
    const size_t need = slime_gemm_ksplit_workspace_bytes(a->M, a->N, splits);
    SLIME_REQUIRE(need < (1ull << 32), "gemm_ksplit: %zu B of partial products (splits=%d x %d padded rows x N=%d fp32) reach the 4 GiB the "
                                       "kernels' 32-bit offsets cover", need, splits, (a->M + 127) / 128 * 128, a->N);
    if (!ws || ws_bytes < need || ((uintptr_t)ws % 256) != 0) {
        slime_set_error("gemm_ksplit: workspace %zu B (need %zu, 256-B aligned)", ws_bytes, need);
        return SLIME_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    if (a->dtype == SLIME_BF16) return launch_ksplit_T<BF16>(g, a->epilogue, (char*)ws, splits, s);
    return launch_ksplit_T<F16>(g, a->epilogue, (char*)ws, splits, s);
}
