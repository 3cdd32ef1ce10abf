// attention_diag.inc -- everything of the attention that exists in the DIAGNOSTIC build only (libslime_hip_diag.so, -DSLIME_DIAG:
// tools/ and the variant-forcing tests).  Included by attention.hip under SLIME_DIAG, after the product kernels and launchers
// (shares AttnArgs, attn64_body, attn64r_pass and launch_attn64r) and before slime_attention.
//   * the measured-alternative CLIP kernels attn64_kernel (round 1), attn64w_kernel (twelve waves), attn64g_kernel (K/V ring) and
//     attention32.inc (one wave per SIMD on 32x32x16 MFMAs), with their launchers;
//   * the process-global hooks and their setters;
//   * diag_attention, the one call slime_attention makes into this file.
#include <optional>

// attn64_kernel (round 1): two workgroups per (crop, head), two DMA halves -- attn64_body in attention.hip.
template <typename T>
__global__ void __launch_bounds__(512) attn64_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = 8;
    const int h = blockIdx.x, b = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int total_sb = (a.n_q + 15) >> 4;
    const int wg_sb0 = blockIdx.z * a.sb_per_wg;
    const int nsb = min(a.sb_per_wg, total_sb - wg_sb0);
    const int base = nsb / NW, rem = nsb % NW;
    const int cnt = base + (wave < rem ? 1 : 0);
    const int sb0 = wg_sb0 + wave * base + min(wave, rem);
    switch (cnt) {
        case 0: attn64_body<T, 0>(a, smem, b, h, sb0); break;
        case 1: attn64_body<T, 1>(a, smem, b, h, sb0); break;
        case 2: attn64_body<T, 2>(a, smem, b, h, sb0); break;
        default: attn64_body<T, 3>(a, smem, b, h, sb0); break;
    }
}

template <typename T>
static int launch_attn64(const AttnArgs& a0, int batch, hipStream_t stream) {
    AttnArgs a = a0;
    constexpr int LDS = 2 * 608 * 128;
    auto kern = attn64_kernel<T>;
    SLIME_SET_LDS_ONCE(kern, LDS, "attention");
    const int total_sb = (a.n_q + 15) / 16;
    const int qsplit = (total_sb + 23) / 24;                  // <= 3 sub-blocks per wave, 8 waves
    a.sb_per_wg = (total_sb + qsplit - 1) / qsplit;
    hipLaunchKernelGGL(kern, dim3(a.heads, batch, qsplit), dim3(512), LDS, stream, a);
    SLIME_CHECK_LAUNCH("attention64");
    return SLIME_OK;
}

// Twelve-wave variant: three waves per SIMD (<= 2 sub-blocks each, <= 168 VGPRs) instead of two with three sub-blocks.
// rocprofv3 on attn64r: 36 % of the wave cycles are parked at s_waitcnt / s_barrier and 33 % stalled at issue -- latency, not
// throughput -- so the third wave per SIMD is there to cover the other two's waits.  24 sub-blocks per workgroup at most,
// i.e. always two workgroups per CLIP (crop, head); pass 1 only.
template <typename T>
__global__ void __launch_bounds__(768) attn64w_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = 12;
    const int h = blockIdx.x, b = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int total_sb = (a.n_q + 15) >> 4;
    const int wg_sb0 = blockIdx.z * a.sb_per_wg;
    const int nsb = min(a.sb_per_wg, total_sb - wg_sb0);      // <= 2 * NW
    const int base = nsb / NW, rem = nsb % NW;
    const int cnt = base + (wave < rem ? 1 : 0);
    const int sb0 = wg_sb0 + wave * base + min(wave, rem);
    switch (cnt) {
        case 0: attn64r_pass<T, 0, false, NW, false>(a, smem, b, h, sb0); break;
        case 1: attn64r_pass<T, 1, false, NW, false>(a, smem, b, h, sb0); break;
        default: attn64r_pass<T, 2, false, NW, false>(a, smem, b, h, sb0); break;
    }
}

template <typename T>
static int launch_attn64w(const AttnArgs& a0, int batch, hipStream_t stream) {
    AttnArgs a = a0;
    constexpr int LDS = 2 * 608 * 128;
    auto kern = attn64w_kernel<T>;
    SLIME_SET_LDS_ONCE(kern, LDS, "attention");
    const int total_sb = (a.n_q + 15) / 16;
    const int qsplit = (total_sb + 23) / 24;
    a.sb_per_wg = (total_sb + qsplit - 1) / qsplit;
    hipLaunchKernelGGL(kern, dim3(a.heads, batch, qsplit), dim3(768), LDS, stream, a);
    SLIME_CHECK_LAUNCH("attention64w");
    return SLIME_OK;
}

// ================================================================================================
// attn64g_kernel (round 4, measured alternative): the same pass on a K/V RING -- four waves, 2 x 32 KiB of LDS, <= 256 registers --
// so that an attention workgroup no longer monopolises its CU (attn64r: 152 KiB + 8 waves x 245 registers) but can share it with
// another attention workgroup or with a direct-B GEMM workgroup of the tower's other stream (4 waves x 256 registers, 33 KiB):
// VALU / LDS-heavy softmax waves beside MFMA / L2-bound GEMM waves.  12 query sub-blocks per workgroup (3 per wave), i.e. four
// workgroups per CLIP (crop, head), each streaming the whole K/V once through the ring (granule = 32 rows = one step, 8 slots,
// 4 ahead).  One-dimensional grid: the four workgroups of an item are 8 apart in launch order -- same XCD, same L2 -- and items
// of 8 consecutive heads fill the 8 XCDs.  Same arithmetic in the same order per query sub-block: bit-identical to attn64r.
// Measured (tools/attn_ring_ab.py, profiles/r04_attention_ring.txt): stand-alone 52 -> 46-48 us at 20 crops, 87 -> 81-83 at 40,
// 16 -> 13.4 at one crop, equal at 5-9; the two-stream tower 15.28-15.34 -> 15.51-15.52 ms (SLOWER), one stream equal.  Like attn32
// in rounds 2-3: under the power cap a faster attention that does the same work moves the step nowhere.  Diagnostic build only.
// ================================================================================================
template <typename T>
__global__ void __launch_bounds__(256, 2) attn64g_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = 4, AHEAD = 4, RING = 256;
    const int qsplit = a.sb_per_wg >> 16, sb_per_wg = a.sb_per_wg & 0xffff;
    // launch index -> (item, split): id = 8 qsplit (item / 8) + 8 split + item % 8
    const int id = blockIdx.x, grp = id / (8 * qsplit), rem = id % (8 * qsplit);
    const int item = grp * 8 + (rem & 7), split = rem >> 3;
    if (item >= a.n_items) return;                            // the grid is padded to whole groups of 8 items
    const int h = item % a.heads, b = item / a.heads;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int total_sb = (a.n_q + 15) >> 4;
    const int wg_sb0 = split * sb_per_wg;
    const int nsb = max(0, min(sb_per_wg, total_sb - wg_sb0));     // <= 3 * NW
    const int base = nsb / NW, rm = nsb % NW;
    const int cnt = base + (wave < rm ? 1 : 0);
    const int sb0 = wg_sb0 + wave * base + min(wave, rm);
    switch (cnt) {
        case 0: attn64r_pass<T, 0, false, NW, false, AHEAD, RING>(a, smem, b, h, sb0); break;
        case 1: attn64r_pass<T, 1, false, NW, false, AHEAD, RING>(a, smem, b, h, sb0); break;
        case 2: attn64r_pass<T, 2, false, NW, false, AHEAD, RING>(a, smem, b, h, sb0); break;
        default: attn64r_pass<T, 3, false, NW, false, AHEAD, RING>(a, smem, b, h, sb0); break;
    }
}

template <typename T>
static int launch_attn64g(const AttnArgs& a0, int batch, hipStream_t stream) {
    AttnArgs a = a0;
    constexpr int LDS = 2 * 256 * 128;
    auto kern = attn64g_kernel<T>;
    SLIME_SET_LDS_ONCE(kern, LDS, "attention");
    const int total_sb = (a.n_q + 15) / 16;
    const int qsplit = (total_sb + 11) / 12;                  // <= 3 sub-blocks per wave, 4 waves
    const int per = (total_sb + qsplit - 1) / qsplit;
    a.sb_per_wg = (qsplit << 16) | per;
    a.n_items = a.heads * batch;
    const int groups = (a.n_items + 7) / 8;
    hipLaunchKernelGGL(kern, dim3(groups * 8 * qsplit), dim3(256), LDS, stream, a);
    SLIME_CHECK_LAUNCH("attention64g");
    return SLIME_OK;
}

#include "attention32.inc"

// Process-global hooks.  The product library has no mutable globals.
static unsigned long long* g_attn_dbg = nullptr;
static int g_attn_abl = 0;
extern "C" void slime_attention_set_ablation(int v) { g_attn_abl = v; }
static int g_attn_variant = 0;      // 1 = force the generic kernel
extern "C" void slime_attention_set_variant(int v) { g_attn_variant = v; }
extern "C" void slime_attention_set_debug(void* p) { g_attn_dbg = (unsigned long long*)p; }

// The diagnostic part of slime_attention: fills the hook fields of the argument block and walks the forced variants.  Returns the
// launch status of the variant it ran.  Without a value, slime_attention goes on: to the product's CLIP kernel, or -- clip_shape
// cleared: a forced variant (1 = the generic kernel) or a stamp buffer that no branch here takes -- to the generic kernel.
static std::optional<int> diag_attention(AttnArgs& a, bool& clip_shape, int batch, int head_dim, int n_kv, int dtype, hipStream_t s) {
    a.dbg = g_attn_dbg; a.abl = g_attn_abl;
    if (g_attn_variant != 0 || g_attn_dbg) clip_shape = false;
    if (head_dim == 64 && n_kv <= 608 && n_kv >= 321 && g_attn_variant >= 4 && g_attn_variant <= 6 && dtype == SLIME_BF16)
        return launch_attn32<BF16>(a, batch, g_attn_variant == 5 ? 2 : g_attn_variant == 6 ? -1 : 0, s);
    if (head_dim == 64 && n_kv <= 608 && n_kv >= 321 && g_attn_variant >= 12 && g_attn_variant <= 15 && dtype == SLIME_BF16)
        return launch_attn32<BF16>(a, batch, g_attn_variant - 10, s);                       // every item cut in 2 / 3 / 4 / 5
    if (head_dim == 64 && n_kv <= 608 && n_kv >= 321 && g_attn_variant >= 22 && g_attn_variant <= 27 && dtype == SLIME_BF16) {
        // attn64r with 2 / 3 / 4 / 6 K/V granules requested ahead, 27: the whole panel up front (rounds 1-2); with or without stamp records
        switch (g_attn_variant) {
            case 22: return launch_attn64r<BF16, 2>(a, batch, s);
            case 23: return launch_attn64r<BF16, 3>(a, batch, s);
            case 24: return launch_attn64r<BF16, 4>(a, batch, s);
            case 26: return launch_attn64r<BF16, 6>(a, batch, s);
            default: return launch_attn64r<BF16, 16>(a, batch, s);
        }
    }
    if (head_dim == 64 && n_kv <= 608 && n_kv >= 321 && g_attn_variant == 40 && dtype == SLIME_BF16 && !g_attn_dbg)
        return launch_attn64r<BF16, 3, 1>(a, batch, s);      // round 6 timing ablation: conflict-free plain reads instead of the V^T transpose reads (wrong results)
    if (head_dim == 64 && n_kv <= 608 && n_kv >= 321 && g_attn_variant == 17 && g_attn_dbg) {   // attn64r with one stamp record per workgroup
        if (dtype == SLIME_F16) return launch_attn64r<F16>(a, batch, s);
        return launch_attn64r<BF16>(a, batch, s);
    }
    if (head_dim == 64 && n_kv <= 608 && n_kv >= 321 && g_attn_variant == 7 && !g_attn_dbg) {    // round 2's product kernel, for A/B
        if (dtype == SLIME_F16) return launch_attn64r<F16>(a, batch, s);
        return launch_attn64r<BF16>(a, batch, s);
    }
    if (head_dim == 64 && n_kv <= 608 && n_kv >= 321 && g_attn_variant == 30 && !g_attn_dbg) {   // round 4: K/V ring, four waves, two per CU
        if (dtype == SLIME_F16) return launch_attn64g<F16>(a, batch, s);
        return launch_attn64g<BF16>(a, batch, s);
    }
    if (head_dim == 64 && n_kv <= 608 && n_kv >= 321 && g_attn_variant == 3 && !g_attn_dbg) {
        if (dtype == SLIME_F16) return launch_attn64w<F16>(a, batch, s);
        return launch_attn64w<BF16>(a, batch, s);
    }
    if (head_dim == 64 && n_kv <= 608 && n_kv >= 321 && g_attn_variant == 2 && !g_attn_dbg) {
        // the round-1 kernel (two workgroups per (crop, head), two DMA halves), kept for A/B
        if (dtype == SLIME_F16) return launch_attn64<F16>(a, batch, s);
        return launch_attn64<BF16>(a, batch, s);
    }
    return std::nullopt;
}
