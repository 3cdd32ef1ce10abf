// slicer.hip -- the resampling half of the SliME image slicer on the GPU (gfx950).
//
// Pillow's ImagingResample (8 bpc) restated for the device: the weights are produced on the host in double
// precision exactly as Pillow does (precompute_coeffs + normalize_coeffs_8bpc; contraction off so no fma
// sneaks in), the two passes run here in 32-bit integer arithmetic.  Both kernels are HBM/L2 streaming
// kernels over a few MB: the vertical pass is perfectly coalesced (a thread owns one byte column), the
// horizontal pass stages the source span of a 256-pixel output segment in LDS with 16-byte loads.
#include "common.h"
#include <math.h>
#include <stdlib.h>

namespace {
constexpr int PRECISION_BITS = 32 - 8 - 2;

#pragma clang fp contract(off)
inline double bicubic_weight(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Pillow's lanczos_filter (support 3.0)
inline double sinc_weight(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
inline double lanczos_weight(double x) {
    if (-3.0 <= x && x < 3.0) return sinc_weight(x) * sinc_weight(x / 3);
    return 0.0;
}
inline bool known_filter(int filter) { return filter == SLIME_FILTER_BICUBIC || filter == SLIME_FILTER_LANCZOS; }
inline double filter_support(int filter) { return filter == SLIME_FILTER_LANCZOS ? 3.0 : 2.0; }

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> PRECISION_BITS;
    return (uint8_t)min(max(v, 0), 255);
}

// Horizontal pass.  One workgroup = one source row x SEG output pixels.  LDS holds the source bytes the
// segment needs ([xmin(first), xmin(last)+count(last)) x 3), fetched 16 B per lane; spans that do not fit
// (extreme down-scales) are read from global memory directly.
constexpr int SEG = 256, SPAN_BYTES = 48 * 1024;
// One output segment of one source row (shared by the single-size and the job-table kernel): `row` = the source row, `drow` = the
// destination row, [src_begin, src_end) = the allocation the 16-byte staging loads must stay inside.
__device__ __forceinline__ void resample_h_segment(uint8_t* span, const uint8_t* row, const uint8_t* src_begin, const uint8_t* src_end,
                                                   uint8_t* drow, int x0, int out_w, const int* __restrict__ bounds,
                                                   const int* __restrict__ kk, int ksize) {
    const int x1 = min(x0 + SEG, out_w) - 1;
    const int first = bounds[2 * x0], last = bounds[2 * x1] + bounds[2 * x1 + 1];     // source pixels [first, last)
    // stage [g0, g1): g0 = the 16-B aligned address at or below the first needed byte (absolute alignment: rows of
    // a packed RGB image are not 16-B aligned themselves)
    const uint8_t* need0 = row + (size_t)first * 3;
    const uint8_t* g1 = row + (size_t)last * 3;
    const uint8_t* g0 = reinterpret_cast<const uint8_t*>(reinterpret_cast<size_t>(need0) & ~(size_t)15);
    const bool staged = (g1 - g0) <= SPAN_BYTES;
    if (staged) {
        for (const uint8_t* g = g0 + threadIdx.x * 16; g < g1; g += 256 * 16) {
            if (g >= src_begin && g + 16 <= src_end) {
                *reinterpret_cast<u32x4*>(span + (g - g0)) = *reinterpret_cast<const u32x4*>(g);
            } else {
                for (int i = 0; i < 16; ++i)
                    if (g + i >= src_begin && g + i < src_end) span[g - g0 + i] = g[i];
            }
        }
        __syncthreads();
    }
    const int x = x0 + threadIdx.x;
    if (x >= out_w) return;
    const int xmin = bounds[2 * x], cnt = bounds[2 * x + 1];
    const int* k = kk + (size_t)x * ksize;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    if (staged) {
        const uint8_t* p = span + (row + (size_t)xmin * 3 - g0);
        for (int t = 0; t < cnt; ++t) {
            const int w = k[t];
            s0 += p[3 * t] * w; s1 += p[3 * t + 1] * w; s2 += p[3 * t + 2] * w;
        }
    } else {
        const uint8_t* p = row + (size_t)xmin * 3;
        for (int t = 0; t < cnt; ++t) {
            const int w = k[t];
            s0 += p[3 * t] * w; s1 += p[3 * t + 1] * w; s2 += p[3 * t + 2] * w;
        }
    }
    uint8_t* d = drow + (size_t)x * 3;
    d[0] = clip8(s0); d[1] = clip8(s1); d[2] = clip8(s2);
}

__global__ void __launch_bounds__(256) resample_h_kernel(const uint8_t* __restrict__ src, long src_image_stride, long src_stride,
                                                         int src_w, const uint8_t* src_begin, const uint8_t* src_end,
                                                         uint8_t* __restrict__ dst, long dst_image_stride, long dst_stride, int out_w,
                                                         const int* __restrict__ bounds, const int* __restrict__ kk, int ksize) {
    __shared__ __attribute__((aligned(16))) uint8_t span[SPAN_BYTES];
    const int y = blockIdx.y;
    const uint8_t* row = src + (size_t)blockIdx.z * src_image_stride + (size_t)y * src_stride;
    resample_h_segment(span, row, src_begin, src_end, dst + (size_t)blockIdx.z * dst_image_stride + (size_t)y * dst_stride,
                       blockIdx.x * SEG, out_w, bounds, kk, ksize);
}

// Vertical pass: a thread owns 4 consecutive bytes of an output row (x*3+c is just a byte column for this
// pass), taps walk down the source rows -> every load/store of a wave is one contiguous 256-B segment.
__global__ void __launch_bounds__(256) resample_v_kernel(const uint8_t* __restrict__ src, long src_image_stride, long src_stride,
                                                         uint8_t* __restrict__ dst, long dst_image_stride, long dst_stride, int row_bytes,
                                                         const int* __restrict__ bounds, const int* __restrict__ kk, int ksize) {
    const int y = blockIdx.y;
    const int c = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (c >= row_bytes) return;
    src += (size_t)blockIdx.z * src_image_stride;
    dst += (size_t)blockIdx.z * dst_image_stride;
    const int ymin = bounds[2 * y], cnt = bounds[2 * y + 1];
    const int* k = kk + (size_t)y * ksize;
    int s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = 1 << (PRECISION_BITS - 1);
    const bool full = c + 4 <= row_bytes && ((src_stride | (size_t)src) & 3) == 0;
    for (int t = 0; t < cnt; ++t) {
        const uint8_t* p = src + (size_t)(ymin + t) * src_stride + c;
        const int w = k[t];
        if (full) {
            const unsigned v = *reinterpret_cast<const unsigned*>(p);
            s[0] += (int)(v & 255u) * w; s[1] += (int)((v >> 8) & 255u) * w;
            s[2] += (int)((v >> 16) & 255u) * w; s[3] += (int)(v >> 24) * w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) if (c + i < row_bytes) s[i] += p[i] * w;
        }
    }
    uint8_t* d = dst + (size_t)y * dst_stride + c;
#pragma unroll
    for (int i = 0; i < 4; ++i) if (c + i < row_bytes) d[i] = clip8(s[i]);
}

// ---- job table (slime_slice_jobs): a whole batch of differently sized images in two launches ----------------------------------------
template <typename T> __device__ __forceinline__ unsigned short to_t1(float x) {
    return (unsigned short)(T::pack2(x, 0.f) & 0xffffu);
}

// The job a workgroup belongs to: the last one whose first workgroup index is <= block (jobs without workgroups in this launch
// repeat their successor's index, so they are never picked).
template <bool V, typename Job> __device__ __forceinline__ int job_of_block(const Job* __restrict__ jobs, int n_jobs, int block) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((V ? jobs[mid].v_block0 : jobs[mid].h_block0) <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Launch 1: resample_h_kernel for every job that runs both passes, into the job's intermediate [src_h, out_w, 3] at tmp + tmp_offset.
// The staging loads are bounded by the job's OWN source allocation.
__global__ void __launch_bounds__(256) slice_h_kernel(const slime_slice_job* __restrict__ jobs, int n_jobs, uint8_t* __restrict__ tmp) {
    __shared__ __attribute__((aligned(16))) uint8_t span[SPAN_BYTES];
    const slime_slice_job& J = jobs[job_of_block<false>(jobs, n_jobs, blockIdx.x)];
    const int segs = (J.out_w + SEG - 1) / SEG, local = blockIdx.x - J.h_block0;
    const int y = local / segs, x0 = (local % segs) * SEG;
    const uint8_t* src_end = J.src + (size_t)(J.src_h - 1) * J.src_stride + (size_t)J.src_w * 3;
    resample_h_segment(span, J.src + (size_t)y * J.src_stride, J.src, src_end, tmp + J.tmp_offset + (size_t)y * J.out_w * 3, x0, J.out_w,
                       J.bounds_h, J.kk_h, J.ksize_h);
}

// Launch 2: vertical pass + paste + tile + normalise.  A workgroup owns one canvas row of one tile (the unit of tile_normalize_kernel):
// a thread produces 4 consecutive bytes of the canvas row -- resample_v_kernel's taps over the intermediate (both passes) or the source
// (equal widths), a copy (equal heights and widths), the horizontal taps read straight from the source row (equal heights: the row
// is final, it needs no intermediate), 0 outside the paste rectangle -- into LDS, and the interleaved line leaves as three planar
// channel rows of normalised values.  4-byte loads only where all 4 bytes lie inside the resized row, so nothing outside the job's
// allocation is touched.
template <typename T>
__global__ void __launch_bounds__(256) slice_v_tile_kernel(const slime_slice_job* __restrict__ jobs, int n_jobs, int crop,
                                                           const uint8_t* __restrict__ tmp, float3 mean, float3 sd, void* out,
                                                           int out_dtype) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint8_t* line = reinterpret_cast<uint8_t*>(smem);
    const slime_slice_job& J = jobs[job_of_block<true>(jobs, n_jobs, blockIdx.x)];
    const int local = blockIdx.x - J.v_block0, tiles_x = J.canvas_w / crop;
    const int y = local % crop, tile = local / crop;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int oy = ty * crop + y - J.y0;                                   // row of the resized image, if inside [0, out_h)
    const int row_bytes = J.out_w * 3, seg_bytes = crop * 3;
    const int sb0 = (tx * crop - J.x0) * 3;                                // byte column of the resized row at the segment's start
    const bool need_h = J.out_w != J.src_w, need_v = J.out_h != J.src_h;
    const uint8_t* vsrc = J.src;                                           // the rows the vertical taps (or the copy) read
    long vstride = J.src_stride;
    if (need_h && need_v) { vsrc = tmp + J.tmp_offset; vstride = row_bytes; }
    if (oy >= 0 && oy < J.out_h) {
        int ymin = oy, cnt = 1;
        const int* k = nullptr;
        if (need_v) { ymin = J.bounds_v[2 * oy]; cnt = J.bounds_v[2 * oy + 1]; k = J.kk_v + (size_t)oy * J.ksize_v; }
        for (int i = threadIdx.x * 4; i < seg_bytes; i += 1024) {
            const int sb = sb0 + i, nb = min(4, seg_bytes - i);
            uint8_t r[4] = {0, 0, 0, 0};
            if (sb + nb > 0 && sb < row_bytes) {
                const uint8_t* p = vsrc + ((long)ymin * vstride + sb);
                const bool full = nb == 4 && sb >= 0 && sb + 4 <= row_bytes && ((vstride | (size_t)p) & 3) == 0;
                if (need_v) {
                    int s[4];
#pragma unroll
                    for (int b = 0; b < 4; ++b) s[b] = 1 << (PRECISION_BITS - 1);
                    for (int t = 0; t < cnt; ++t, p += vstride) {
                        const int w = k[t];
                        if (full) {
                            const unsigned v = *reinterpret_cast<const unsigned*>(p);
                            s[0] += (int)(v & 255u) * w; s[1] += (int)((v >> 8) & 255u) * w;
                            s[2] += (int)((v >> 16) & 255u) * w; s[3] += (int)(v >> 24) * w;
                        } else {
#pragma unroll
                            for (int b = 0; b < 4; ++b) if (b < nb && sb + b >= 0 && sb + b < row_bytes) s[b] += p[b] * w;
                        }
                    }
#pragma unroll
                    for (int b = 0; b < 4; ++b) if (b < nb && sb + b >= 0 && sb + b < row_bytes) r[b] = clip8(s[b]);
                } else if (need_h) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if (b < nb && sb + b >= 0 && sb + b < row_bytes) {
                            const int x = (sb + b) / 3, c = (sb + b) % 3;
                            const int xmin = J.bounds_h[2 * x], n = J.bounds_h[2 * x + 1];
                            const int* kh = J.kk_h + (size_t)x * J.ksize_h;
                            const uint8_t* q = J.src + (size_t)oy * J.src_stride + (size_t)xmin * 3 + c;
                            int acc = 1 << (PRECISION_BITS - 1);
                            for (int t = 0; t < n; ++t) acc += q[3 * t] * kh[t];
                            r[b] = clip8(acc);
                        }
                    }
                } else if (full) {
                    const unsigned v = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
                    for (int b = 0; b < 4; ++b) r[b] = (uint8_t)(v >> (8 * b));
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b) if (b < nb && sb + b >= 0 && sb + b < row_bytes) r[b] = p[b];
                }
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) if (b < nb) line[i + b] = r[b];                // nb < 4 only at the end of a line whose crop % 4 != 0
        }
    } else {
        for (int i = threadIdx.x; i < seg_bytes; i += 256) line[i] = 0;
    }
    __syncthreads();
    const float m[3] = {mean.x, mean.y, mean.z}, sdv[3] = {sd.x, sd.y, sd.z};
    for (int i = threadIdx.x; i < seg_bytes; i += 256) {
        const int c = i / crop, x = i % crop;
        // tile_normalize_kernel's expression (HF rescale = float32(float64(u8) * (1/255)), normalise = (x - mean) / std in fp32)
        const float v = ((float)((double)line[x * 3 + c] * (1.0 / 255.0)) - m[c]) / sdv[c];
        const size_t o = ((((size_t)J.first_crop + tile) * 3 + c) * crop + y) * crop + x;
        if (out_dtype == SLIME_F32) reinterpret_cast<float*>(out)[o] = v;
        else reinterpret_cast<unsigned short*>(out)[o] = to_t1<T>(v);
    }
}

// What slime_slice_jobs_plan fills in, computed without touching the table: slime_slice_jobs compares the table against it.
struct SlicePlan { long tmp_offset[SLIME_SLICE_MAX_JOBS]; int h_block0[SLIME_SLICE_MAX_JOBS], v_block0[SLIME_SLICE_MAX_JOBS];
                   size_t tmp_bytes; long h_blocks, v_blocks; };
int slice_plan(const slime_slice_job* jobs, int n_jobs, int crop, SlicePlan* p) {
    SLIME_REQUIRE(jobs && crop > 0, "slice_jobs: null job table or crop %d", crop);
    SLIME_REQUIRE(n_jobs >= 1 && n_jobs <= SLIME_SLICE_MAX_JOBS, "slice_jobs: %d jobs (1 .. SLIME_SLICE_MAX_JOBS = %d)", n_jobs, SLIME_SLICE_MAX_JOBS);
    size_t tmp = 0;
    long hb = 0, vb = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const slime_slice_job& J = jobs[j];
        SLIME_REQUIRE(J.src_h > 0 && J.src_w > 0 && J.out_h > 0 && J.out_w > 0, "slice_jobs: job %d: empty image (%dx%d -> %dx%d)", j, J.src_h, J.src_w, J.out_h, J.out_w);
        SLIME_REQUIRE(J.canvas_h > 0 && J.canvas_w > 0 && J.canvas_h % crop == 0 && J.canvas_w % crop == 0,
                      "slice_jobs: job %d: canvas %dx%d is not a multiple of crop %d", j, J.canvas_h, J.canvas_w, crop);
        const bool both = J.out_w != J.src_w && J.out_h != J.src_h;
        p->tmp_offset[j] = both ? (long)tmp : 0;
        p->h_block0[j] = (int)hb;
        p->v_block0[j] = (int)vb;
        if (both) {
            tmp += align_up((size_t)J.src_h * J.out_w * 3, 16);
            hb += (long)((J.out_w + SEG - 1) / SEG) * J.src_h;
        }
        vb += (long)J.canvas_h * (J.canvas_w / crop);
        SLIME_REQUIRE(hb < (1L << 31) && vb < (1L << 31), "slice_jobs: more than 2^31 - 1 workgroups in one launch at job %d", j);
    }
    p->tmp_bytes = tmp; p->h_blocks = hb; p->v_blocks = vb;
    return SLIME_OK;
}

// ---- view jobs (slime_view_jobs): pad first, resize with either filter, cut windows -- the other process_images modes ---------------
// The virtual source of a job is its FIELD: field_h x field_w pixels of colour bg with the box of the image pasted at (paste_x, paste_y).
// Integer sums do not depend on their order, so a tap row is split into the taps that fall on bg (their weights are summed and
// multiplied by the colour once) and the run of taps that fall on the box (read as the kernels above read them).
__device__ __forceinline__ int view_h_cols(const slime_view_job& J, int crop) { return (J.win_nx - 1) * J.win_step + crop; }

// One output segment of one FIELD row fy: resample_h_segment with the field's padding.  The staged span is the part of the BOX row the
// segment needs; the 16-byte staging loads are bounded by the job's image allocation.  Columns [x0, min(x0 + SEG, x_end)).
__device__ __forceinline__ void view_h_segment(uint8_t* span, const slime_view_job& J, int fy, uint8_t* drow, int x0, int x_end) {
    const int* __restrict__ bounds = J.bounds_h;
    const int ksize = J.ksize_h;
    const int x1 = min(x0 + SEG, x_end) - 1;
    const int px0 = J.paste_x, px1 = J.paste_x + J.box_w;
    const bool in_rows = fy >= J.paste_y && fy < J.paste_y + J.box_h;                 // else the whole field row is bg
    // row + fx * 3 = the pixel under field column fx, for px0 <= fx < px1
    const uint8_t* row = J.img + (in_rows ? (long)(J.box_y0 + fy - J.paste_y) * J.img_stride + ((long)J.box_x0 - px0) * 3 : 0L);
    const int first = max(bounds[2 * x0], px0), last = min(bounds[2 * x1] + bounds[2 * x1 + 1], px1);   // box pixels [first, last)
    const uint8_t* g0 = row;
    bool staged = false;
    if (in_rows && first < last) {                                                   // uniform over the workgroup
        const uint8_t* src_end = J.img + (size_t)(J.img_h - 1) * J.img_stride + (size_t)J.img_w * 3;
        const uint8_t* g1 = row + (long)last * 3;
        g0 = reinterpret_cast<const uint8_t*>(reinterpret_cast<size_t>(row + (long)first * 3) & ~(size_t)15);
        staged = (g1 - g0) <= SPAN_BYTES;
        if (staged) {
            for (const uint8_t* g = g0 + threadIdx.x * 16; g < g1; g += 256 * 16) {
                if (g >= J.img && g + 16 <= src_end) {
                    *reinterpret_cast<u32x4*>(span + (g - g0)) = *reinterpret_cast<const u32x4*>(g);
                } else {
                    for (int i = 0; i < 16; ++i)
                        if (g + i >= J.img && g + i < src_end) span[g - g0 + i] = g[i];
                }
            }
            __syncthreads();
        }
    }
    const int x = x0 + threadIdx.x;
    if (x >= x_end) return;
    const int xmin = bounds[2 * x], cnt = bounds[2 * x + 1];
    const int* k = J.kk_h + (size_t)x * ksize;
    int a = xmin + cnt, b = xmin + cnt;                                               // taps [a, b) fall on the box
    if (in_rows) { a = min(max(px0, xmin), xmin + cnt); b = min(max(px1, a), xmin + cnt); }
    int wbg = 0;
    for (int t = 0; t < a - xmin; ++t) wbg += k[t];
    for (int t = b - xmin; t < cnt; ++t) wbg += k[t];
    int s0 = (1 << (PRECISION_BITS - 1)) + J.bg[0] * wbg, s1 = (1 << (PRECISION_BITS - 1)) + J.bg[1] * wbg,
        s2 = (1 << (PRECISION_BITS - 1)) + J.bg[2] * wbg;
    const uint8_t* p = staged ? span + (row + (long)a * 3 - g0) : row + (long)a * 3;
    for (int t = a - xmin; t < b - xmin; ++t, p += 3) {
        const int w = k[t];
        s0 += p[0] * w; s1 += p[1] * w; s2 += p[2] * w;
    }
    uint8_t* d = drow + (size_t)x * 3;
    d[0] = clip8(s0); d[1] = clip8(s1); d[2] = clip8(s2);
}

// Launch 1: the horizontal pass of every job that runs both passes, over the columns its windows cover, into the job's intermediate
// [field_h, out_w, 3] at tmp + tmp_offset.
__global__ void __launch_bounds__(256) view_h_kernel(const slime_view_job* __restrict__ jobs, int n_jobs, int crop, uint8_t* __restrict__ tmp) {
    __shared__ __attribute__((aligned(16))) uint8_t span[SPAN_BYTES];
    const slime_view_job& J = jobs[job_of_block<false>(jobs, n_jobs, blockIdx.x)];
    const int cols = view_h_cols(J, crop), segs = (cols + SEG - 1) / SEG, local = blockIdx.x - J.h_block0;
    const int fy = local / segs, x0 = J.win_x0 + (local % segs) * SEG;
    view_h_segment(span, J, fy, tmp + J.tmp_offset + (size_t)fy * J.out_w * 3, x0, J.win_x0 + cols);
}

// 4 bytes (nb of them used) of field row fy at byte column sb, packed little-endian: the box where it covers them, bg elsewhere.
// A 4-byte load only where all four bytes lie inside the box (so inside the image) and the address is aligned.
__device__ __forceinline__ unsigned view_field4(const slime_view_job& J, int fy, int sb, int nb, unsigned bgw) {
    const int pb0 = J.paste_x * 3, pb1 = (J.paste_x + J.box_w) * 3;
    if (fy < J.paste_y || fy >= J.paste_y + J.box_h || sb + nb <= pb0 || sb >= pb1) return bgw;
    const uint8_t* p = J.img + ((long)(J.box_y0 + fy - J.paste_y) * J.img_stride + (long)J.box_x0 * 3 + (sb - pb0));
    if (nb == 4 && sb >= pb0 && sb + 4 <= pb1 && ((size_t)p & 3) == 0) return *reinterpret_cast<const unsigned*>(p);
    unsigned v = bgw;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (b < nb && sb + b >= pb0 && sb + b < pb1) v = (v & ~(255u << (8 * b))) | ((unsigned)p[b] << (8 * b));
    return v;
}

// Launch 2: vertical pass + windows + normalise.  A workgroup owns one row of one window; a thread produces 4 consecutive bytes of it
// -- the vertical taps over the intermediate (both passes) or over the field (equal widths), the field itself (equal sizes), the
// horizontal taps over the field row (equal heights: the row is final) -- into LDS, and the interleaved line leaves as three planar
// channel rows of normalised values (slice_v_tile_kernel's expression and rounding).
template <typename T>
__global__ void __launch_bounds__(256) view_v_kernel(const slime_view_job* __restrict__ jobs, int n_jobs, int crop,
                                                     const uint8_t* __restrict__ tmp, float3 mean, float3 sd, void* out, int out_dtype) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint8_t* line = reinterpret_cast<uint8_t*>(smem);
    const slime_view_job& J = jobs[job_of_block<true>(jobs, n_jobs, blockIdx.x)];
    const int local = blockIdx.x - J.v_block0;
    const int y = local % crop, win = local / crop;
    const int oy = J.win_y0 + (win / J.win_nx) * J.win_step + y;                       // row of the resized image
    const int sb0 = (J.win_x0 + (win % J.win_nx) * J.win_step) * 3;                    // its byte column at the window's start
    const int row_bytes = J.out_w * 3, seg_bytes = crop * 3;
    const bool need_h = J.out_w != J.field_w, need_v = J.out_h != J.field_h;
    int ymin = oy, cnt = 1;
    const int* k = nullptr;
    if (need_v) { ymin = J.bounds_v[2 * oy]; cnt = J.bounds_v[2 * oy + 1]; k = J.kk_v + (size_t)oy * J.ksize_v; }
    const uint8_t* inter = tmp + J.tmp_offset;
    for (int i = threadIdx.x * 4; i < seg_bytes; i += 1024) {
        const int sb = sb0 + i, nb = min(4, seg_bytes - i);                            // the window lies inside the row: sb + nb <= row_bytes
        unsigned r = 0;
        if (need_h && !need_v) {
            const int px0 = J.paste_x, px1 = J.paste_x + J.box_w;
            const bool in_rows = oy >= J.paste_y && oy < J.paste_y + J.box_h;
            const uint8_t* row = J.img + (in_rows ? (long)(J.box_y0 + oy - J.paste_y) * J.img_stride + ((long)J.box_x0 - px0) * 3 : 0L);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (b < nb) {
                    const int x = (sb + b) / 3, c = (sb + b) % 3;
                    const int xmin = J.bounds_h[2 * x], n = J.bounds_h[2 * x + 1];
                    const int* kh = J.kk_h + (size_t)x * J.ksize_h;
                    int a0 = xmin + n, a1 = xmin + n;
                    if (in_rows) { a0 = min(max(px0, xmin), xmin + n); a1 = min(max(px1, a0), xmin + n); }
                    int wbg = 0;
                    for (int t = 0; t < a0 - xmin; ++t) wbg += kh[t];
                    for (int t = a1 - xmin; t < n; ++t) wbg += kh[t];
                    int acc = (1 << (PRECISION_BITS - 1)) + J.bg[c] * wbg;
                    const uint8_t* q = row + (long)a0 * 3 + c;
                    for (int t = a0 - xmin; t < a1 - xmin; ++t, q += 3) acc += q[0] * kh[t];
                    r |= (unsigned)clip8(acc) << (8 * b);
                }
            }
        } else if (need_h) {                                                           // both passes: plain bytes of the intermediate
            const uint8_t* p = inter + ((long)ymin * row_bytes + sb);
            const bool full = nb == 4 && ((row_bytes | (size_t)p) & 3) == 0;
            int s[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) s[b] = 1 << (PRECISION_BITS - 1);
            for (int t = 0; t < cnt; ++t, p += row_bytes) {
                const int w = k[t];
                if (full) {
                    const unsigned v = *reinterpret_cast<const unsigned*>(p);
                    s[0] += (int)(v & 255u) * w; s[1] += (int)((v >> 8) & 255u) * w;
                    s[2] += (int)((v >> 16) & 255u) * w; s[3] += (int)(v >> 24) * w;
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b) if (b < nb) s[b] += p[b] * w;
                }
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) if (b < nb) r |= (unsigned)clip8(s[b]) << (8 * b);
        } else {                                                                       // equal widths: the rows are field rows
            const int c0 = sb % 3;
            const unsigned bgw = (unsigned)J.bg[c0] | ((unsigned)J.bg[(c0 + 1) % 3] << 8) | ((unsigned)J.bg[(c0 + 2) % 3] << 16) |
                                 ((unsigned)J.bg[c0] << 24);
            if (need_v) {
                int s[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) s[b] = 1 << (PRECISION_BITS - 1);
                for (int t = 0; t < cnt; ++t) {
                    const int w = k[t];
                    const unsigned v = view_field4(J, ymin + t, sb, nb, bgw);
                    s[0] += (int)(v & 255u) * w; s[1] += (int)((v >> 8) & 255u) * w;
                    s[2] += (int)((v >> 16) & 255u) * w; s[3] += (int)(v >> 24) * w;
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) r |= (unsigned)clip8(s[b]) << (8 * b);
            } else {
                r = view_field4(J, oy, sb, nb, bgw);
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) if (b < nb) line[i + b] = (uint8_t)(r >> (8 * b));   // nb < 4 only at the end of a line whose crop % 4 != 0
    }
    __syncthreads();
    const float m[3] = {mean.x, mean.y, mean.z}, sdv[3] = {sd.x, sd.y, sd.z};
    for (int i = threadIdx.x; i < seg_bytes; i += 256) {
        const int c = i / crop, x = i % crop;
        const float v = ((float)((double)line[x * 3 + c] * (1.0 / 255.0)) - m[c]) / sdv[c];
        const size_t o = ((((size_t)J.first_crop + win) * 3 + c) * crop + y) * crop + x;
        if (out_dtype == SLIME_F32) reinterpret_cast<float*>(out)[o] = v;
        else reinterpret_cast<unsigned short*>(out)[o] = to_t1<T>(v);
    }
}

// What slime_view_jobs_plan fills in, with the checks of a job's geometry: slime_view_jobs compares the table against it.
struct ViewPlan { long tmp_offset[SLIME_VIEW_MAX_JOBS]; int h_block0[SLIME_VIEW_MAX_JOBS], v_block0[SLIME_VIEW_MAX_JOBS];
                  size_t tmp_bytes; long h_blocks, v_blocks; };
int view_plan(const slime_view_job* jobs, int n_jobs, int crop, ViewPlan* p) {
    constexpr int MAX_SIDE = (1 << 30) / 3;                                            // byte columns stay inside an int
    SLIME_REQUIRE(jobs && crop > 0 && crop <= MAX_SIDE, "view_jobs: null job table or crop %d", crop);
    SLIME_REQUIRE(n_jobs >= 1 && n_jobs <= SLIME_VIEW_MAX_JOBS, "view_jobs: %d jobs (1 .. SLIME_VIEW_MAX_JOBS = %d)", n_jobs, SLIME_VIEW_MAX_JOBS);
    size_t tmp = 0;
    long hb = 0, vb = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const slime_view_job& J = jobs[j];
        SLIME_REQUIRE(J.img_h > 0 && J.img_w > 0 && J.box_h > 0 && J.box_w > 0 && J.field_h > 0 && J.field_w > 0 && J.out_h > 0 && J.out_w > 0,
                      "view_jobs: job %d: empty image, box, field or output (image %dx%d, box %dx%d, field %dx%d -> %dx%d)", j, J.img_h, J.img_w,
                      J.box_h, J.box_w, J.field_h, J.field_w, J.out_h, J.out_w);
        SLIME_REQUIRE(J.img_w <= MAX_SIDE && J.img_h <= MAX_SIDE && J.field_w <= MAX_SIDE && J.field_h <= MAX_SIDE && J.out_w <= MAX_SIDE && J.out_h <= MAX_SIDE,
                      "view_jobs: job %d: a side exceeds %d pixels", j, MAX_SIDE);
        SLIME_REQUIRE(J.box_x0 >= 0 && J.box_y0 >= 0 && (long)J.box_x0 + J.box_w <= J.img_w && (long)J.box_y0 + J.box_h <= J.img_h,
                      "view_jobs: job %d: box %dx%d at (%d, %d) leaves the %dx%d image", j, J.box_h, J.box_w, J.box_x0, J.box_y0, J.img_h, J.img_w);
        SLIME_REQUIRE(J.paste_x >= 0 && J.paste_y >= 0 && (long)J.paste_x + J.box_w <= J.field_w && (long)J.paste_y + J.box_h <= J.field_h,
                      "view_jobs: job %d: paste of the %dx%d box at (%d, %d) leaves the %dx%d field", j, J.box_h, J.box_w, J.paste_x, J.paste_y,
                      J.field_h, J.field_w);
        SLIME_REQUIRE(J.win_nx > 0 && J.win_ny > 0 && J.win_step > 0, "view_jobs: job %d: win_nx %d, win_ny %d, win_step %d must be positive", j,
                      J.win_nx, J.win_ny, J.win_step);
        SLIME_REQUIRE(J.win_x0 >= 0 && J.win_y0 >= 0 && (long)J.win_x0 + (long)(J.win_nx - 1) * J.win_step + crop <= J.out_w &&
                      (long)J.win_y0 + (long)(J.win_ny - 1) * J.win_step + crop <= J.out_h,
                      "view_jobs: job %d: %dx%d windows of %d from (%d, %d) at step %d leave the %dx%d resized image", j, J.win_ny, J.win_nx, crop,
                      J.win_x0, J.win_y0, J.win_step, J.out_h, J.out_w);
        SLIME_REQUIRE(known_filter(J.filter), "view_jobs: job %d: filter %d is not SLIME_FILTER_BICUBIC / SLIME_FILTER_LANCZOS", j, J.filter);
        const bool both = J.out_w != J.field_w && J.out_h != J.field_h;
        p->tmp_offset[j] = both ? (long)tmp : 0;
        p->h_block0[j] = (int)hb;
        p->v_block0[j] = (int)vb;
        if (both) {
            tmp += align_up((size_t)J.field_h * J.out_w * 3, 16);
            hb += (long)(((J.win_nx - 1) * J.win_step + crop + SEG - 1) / SEG) * J.field_h;
        }
        const long wins = (long)J.win_nx * J.win_ny;
        if (wins < (1L << 31)) vb += wins * crop;
        SLIME_REQUIRE(wins < (1L << 31) && hb < (1L << 31) && vb < (1L << 31), "view_jobs: more than 2^31 - 1 workgroups in one launch at job %d", j);
    }
    p->tmp_bytes = tmp; p->h_blocks = hb; p->v_blocks = vb;
    return SLIME_OK;
}
}  // namespace

extern "C" int slime_resample_ksize_ex(int in_size, int out_size, int filter) {
    if (in_size <= 0 || out_size <= 0 || !known_filter(filter)) return 0;
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(filter_support(filter) * filterscale) * 2 + 1;
}

extern "C" int slime_resample_ksize(int in_size, int out_size) { return slime_resample_ksize_ex(in_size, out_size, SLIME_FILTER_BICUBIC); }

#pragma clang fp contract(off)
extern "C" int slime_resample_coeffs_ex(int in_size, int out_size, int filter, int* bounds, int* kk) {
    SLIME_REQUIRE(in_size > 0 && out_size > 0 && bounds && kk, "resample_coeffs: bad arguments (%d -> %d)", in_size, out_size);
    SLIME_REQUIRE(known_filter(filter), "resample_coeffs: filter %d is not SLIME_FILTER_BICUBIC / SLIME_FILTER_LANCZOS", filter);
    // Pillow: precompute_coeffs(inSize, 0, inSize, outSize, filter) followed by normalize_coeffs_8bpc
    const bool lanczos = filter == SLIME_FILTER_LANCZOS;
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support(filter) * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    const double ss = 1.0 / filterscale;
    double wstack[4096];
    double* wbuf = ksize <= 4096 ? wstack : (double*)malloc((size_t)ksize * sizeof(double));     // a > 1000-fold down-scale
    SLIME_REQUIRE(wbuf, "resample_coeffs: no memory for %d taps (%d -> %d)", ksize, in_size, out_size);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double arg = (x + xmin - center + 0.5) * ss;
            const double w = lanczos ? lanczos_weight(arg) : bicubic_weight(arg);
            wbuf[x] = w;
            ww += w;
        }
        int* k = kk + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            double w = 0.0;
            if (x < xmax) w = (ww != 0.0) ? wbuf[x] / ww : wbuf[x];
            k[x] = w < 0 ? (int)(-0.5 + w * (1 << PRECISION_BITS)) : (int)(0.5 + w * (1 << PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    if (wbuf != wstack) free(wbuf);
    return SLIME_OK;
}

extern "C" int slime_resample_coeffs(int in_size, int out_size, int* bounds, int* kk) {
    return slime_resample_coeffs_ex(in_size, out_size, SLIME_FILTER_BICUBIC, bounds, kk);
}

extern "C" int slime_resize_bicubic_u8_batched(const uint8_t* src, int images, long src_image_stride, int src_h, int src_w,
                                               long src_stride, uint8_t* dst, long dst_image_stride, long dst_stride, int out_h,
                                               int out_w, const int* bounds_h, const int* kk_h, int ksize_h, const int* bounds_v,
                                               const int* kk_v, int ksize_v, uint8_t* tmp, size_t tmp_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SLIME_REQUIRE(src && dst && src_h > 0 && src_w > 0 && out_h > 0 && out_w > 0, "resize_bicubic_u8: bad arguments");
    SLIME_REQUIRE(images > 0 && images <= 65535, "resize_bicubic_u8: %d images", images);
    SLIME_REQUIRE(src_stride >= (long)src_w * 3 && dst_stride >= (long)out_w * 3, "resize_bicubic_u8: row stride smaller than a row");
    const bool need_h = out_w != src_w, need_v = out_h != src_h;
    SLIME_REQUIRE(!need_h || (bounds_h && kk_h && ksize_h == slime_resample_ksize(src_w, out_w)),
                  "resize_bicubic_u8: horizontal tables missing or ksize %d != %d", ksize_h, slime_resample_ksize(src_w, out_w));
    SLIME_REQUIRE(!need_v || (bounds_v && kk_v && ksize_v == slime_resample_ksize(src_h, out_h)),
                  "resize_bicubic_u8: vertical tables missing or ksize %d != %d", ksize_v, slime_resample_ksize(src_h, out_h));
    if (!need_h && !need_v) {
        for (int b = 0; b < images; ++b) {
            hipError_t e = hipMemcpy2DAsync(dst + (size_t)b * dst_image_stride, dst_stride, src + (size_t)b * src_image_stride, src_stride,
                                            (size_t)src_w * 3, src_h, hipMemcpyDeviceToDevice, stream);
            if (e != hipSuccess) { slime_set_error("resize_bicubic_u8: copy: %s", hipGetErrorString(e)); return SLIME_ELAUNCH; }
        }
        return SLIME_OK;
    }
    const uint8_t* vsrc = src;
    long vstride = src_stride, vimg = src_image_stride;
    if (need_h) {
        uint8_t* hdst = need_v ? tmp : dst;
        const long hstride = need_v ? (long)out_w * 3 : dst_stride;
        const long himg = need_v ? (long)src_h * out_w * 3 : dst_image_stride;
        if (need_v) SLIME_REQUIRE(tmp && tmp_bytes >= (size_t)images * src_h * out_w * 3, "resize_bicubic_u8: tmp needs %zu bytes", (size_t)images * src_h * out_w * 3);
        dim3 grid((out_w + SEG - 1) / SEG, src_h, images);
        const uint8_t* src_end = src + (size_t)(images - 1) * src_image_stride + (size_t)(src_h - 1) * src_stride + (size_t)src_w * 3;
        hipLaunchKernelGGL(resample_h_kernel, grid, dim3(256), 0, stream, src, src_image_stride, src_stride, src_w, src, src_end, hdst, himg,
                           hstride, out_w, bounds_h, kk_h, ksize_h);
        SLIME_CHECK_LAUNCH("resample_h");
        vsrc = hdst;
        vstride = hstride;
        vimg = himg;
    }
    if (need_v) {
        const int row_bytes = out_w * 3;
        dim3 grid((row_bytes + 1023) / 1024, out_h, images);
        hipLaunchKernelGGL(resample_v_kernel, grid, dim3(256), 0, stream, vsrc, vimg, vstride, dst, dst_image_stride, dst_stride, row_bytes,
                           bounds_v, kk_v, ksize_v);
        SLIME_CHECK_LAUNCH("resample_v");
    }
    return SLIME_OK;
}

extern "C" int slime_resize_bicubic_u8(const uint8_t* src, int src_h, int src_w, long src_stride, uint8_t* dst,
                                       long dst_stride, int out_h, int out_w, const int* bounds_h, const int* kk_h,
                                       int ksize_h, const int* bounds_v, const int* kk_v, int ksize_v, uint8_t* tmp,
                                       size_t tmp_bytes, void* stream) {
    return slime_resize_bicubic_u8_batched(src, 1, 0, src_h, src_w, src_stride, dst, 0, dst_stride, out_h, out_w, bounds_h, kk_h, ksize_h,
                                           bounds_v, kk_v, ksize_v, tmp, tmp_bytes, stream);
}

extern "C" int slime_slice_jobs_plan(slime_slice_job* jobs, int n_jobs, int crop, size_t* tmp_bytes) {
    SlicePlan p;
    SLIME_REQUIRE(tmp_bytes, "slice_jobs_plan: null tmp_bytes");
    const int rc = slice_plan(jobs, n_jobs, crop, &p);
    if (rc != SLIME_OK) return rc;
    for (int j = 0; j < n_jobs; ++j) {
        jobs[j].tmp_offset = p.tmp_offset[j];
        jobs[j].h_block0 = p.h_block0[j];
        jobs[j].v_block0 = p.v_block0[j];
    }
    *tmp_bytes = p.tmp_bytes;
    return SLIME_OK;
}

extern "C" int slime_slice_jobs(const slime_slice_job* jobs, const slime_slice_job* jobs_dev, int n_jobs, int crop, const float* mean3,
                                const float* std3, void* out, long out_crops, int out_dtype, uint8_t* tmp, size_t tmp_bytes,
                                void* stream) {
    SLIME_REQUIRE(jobs && jobs_dev && out && mean3 && std3, "slice_jobs: null pointer (the job table is given twice: host and device copy)");
    SLIME_REQUIRE(out_dtype == SLIME_F32 || out_dtype == SLIME_BF16 || out_dtype == SLIME_F16, "slice_jobs: out_dtype %d is not F32 / BF16 / F16", out_dtype);
    SlicePlan p;
    const int rc = slice_plan(jobs, n_jobs, crop, &p);
    if (rc != SLIME_OK) return rc;
    for (int j = 0; j < n_jobs; ++j) {
        const slime_slice_job& J = jobs[j];
        SLIME_REQUIRE(J.src, "slice_jobs: job %d: null source", j);
        SLIME_REQUIRE(J.src_stride >= (long)J.src_w * 3, "slice_jobs: job %d: row stride %ld smaller than a row of %d bytes", j, J.src_stride, J.src_w * 3);
        SLIME_REQUIRE(J.x0 >= 0 && J.y0 >= 0 && (long)J.x0 + J.out_w <= J.canvas_w && (long)J.y0 + J.out_h <= J.canvas_h,
                      "slice_jobs: job %d: paste rectangle %dx%d at (%d, %d) leaves the %dx%d canvas", j, J.out_h, J.out_w, J.x0, J.y0, J.canvas_h, J.canvas_w);
        SLIME_REQUIRE(J.out_w == J.src_w || (J.bounds_h && J.kk_h && J.ksize_h == slime_resample_ksize(J.src_w, J.out_w)),
                      "slice_jobs: job %d: horizontal tables missing or ksize %d != %d", j, J.ksize_h, slime_resample_ksize(J.src_w, J.out_w));
        SLIME_REQUIRE(J.out_h == J.src_h || (J.bounds_v && J.kk_v && J.ksize_v == slime_resample_ksize(J.src_h, J.out_h)),
                      "slice_jobs: job %d: vertical tables missing or ksize %d != %d", j, J.ksize_v, slime_resample_ksize(J.src_h, J.out_h));
        const long tiles = (long)(J.canvas_h / crop) * (J.canvas_w / crop);
        SLIME_REQUIRE(J.first_crop >= 0 && J.first_crop + tiles <= out_crops, "slice_jobs: job %d: crops [%ld, %ld) outside the output's [0, %ld)", j,
                      J.first_crop, J.first_crop + tiles, out_crops);
        for (int i = 0; i < j; ++i) {
            const long ti = (long)(jobs[i].canvas_h / crop) * (jobs[i].canvas_w / crop);
            SLIME_REQUIRE(J.first_crop >= jobs[i].first_crop + ti || jobs[i].first_crop >= J.first_crop + tiles,
                          "slice_jobs: crops of jobs %d and %d overlap ([%ld, %ld) and [%ld, %ld))", i, j, jobs[i].first_crop, jobs[i].first_crop + ti,
                          J.first_crop, J.first_crop + tiles);
        }
        SLIME_REQUIRE(J.tmp_offset == p.tmp_offset[j] && J.h_block0 == p.h_block0[j] && J.v_block0 == p.v_block0[j],
                      "slice_jobs: job %d: tmp_offset / h_block0 / v_block0 are not what slime_slice_jobs_plan sets (plan not run?)", j);
    }
    if (p.tmp_bytes && (!tmp || tmp_bytes < p.tmp_bytes || ((size_t)tmp & 15))) {
        slime_set_error("slice_jobs: tmp needs %zu bytes, 16-byte aligned (got %zu at %p)", p.tmp_bytes, tmp ? tmp_bytes : (size_t)0, (void*)tmp);
        return SLIME_EWORKSPACE;
    }
    if (p.h_blocks) {
        hipLaunchKernelGGL(slice_h_kernel, dim3((unsigned)p.h_blocks), dim3(256), 0, (hipStream_t)stream, jobs_dev, n_jobs, tmp);
        SLIME_CHECK_LAUNCH("slice_h");
    }
    const float3 mean = make_float3(mean3[0], mean3[1], mean3[2]), sd = make_float3(std3[0], std3[1], std3[2]);
    const dim3 grid((unsigned)p.v_blocks), block(256);
    const size_t lds = align_up((size_t)crop * 3, 4);
    if (out_dtype == SLIME_F16) hipLaunchKernelGGL((slice_v_tile_kernel<F16>), grid, block, lds, (hipStream_t)stream, jobs_dev, n_jobs, crop, tmp, mean, sd, out, out_dtype);
    else hipLaunchKernelGGL((slice_v_tile_kernel<BF16>), grid, block, lds, (hipStream_t)stream, jobs_dev, n_jobs, crop, tmp, mean, sd, out, out_dtype);
    SLIME_CHECK_LAUNCH("slice_v_tile");
    return SLIME_OK;
}

extern "C" int slime_view_jobs_plan(slime_view_job* jobs, int n_jobs, int crop, size_t* tmp_bytes) {
    ViewPlan p;
    SLIME_REQUIRE(tmp_bytes, "view_jobs_plan: null tmp_bytes");
    const int rc = view_plan(jobs, n_jobs, crop, &p);
    if (rc != SLIME_OK) return rc;
    for (int j = 0; j < n_jobs; ++j) {
        jobs[j].tmp_offset = p.tmp_offset[j];
        jobs[j].h_block0 = p.h_block0[j];
        jobs[j].v_block0 = p.v_block0[j];
    }
    *tmp_bytes = p.tmp_bytes;
    return SLIME_OK;
}

extern "C" int slime_view_jobs(const slime_view_job* jobs, const slime_view_job* jobs_dev, int n_jobs, int crop, const float* mean3,
                               const float* std3, void* out, long out_crops, int out_dtype, uint8_t* tmp, size_t tmp_bytes, void* stream) {
    SLIME_REQUIRE(jobs && jobs_dev && out && mean3 && std3, "view_jobs: null pointer (the job table is given twice: host and device copy)");
    SLIME_REQUIRE(out_dtype == SLIME_F32 || out_dtype == SLIME_BF16 || out_dtype == SLIME_F16, "view_jobs: out_dtype %d is not F32 / BF16 / F16", out_dtype);
    ViewPlan p;
    const int rc = view_plan(jobs, n_jobs, crop, &p);
    if (rc != SLIME_OK) return rc;
    for (int j = 0; j < n_jobs; ++j) {
        const slime_view_job& J = jobs[j];
        SLIME_REQUIRE(J.img, "view_jobs: job %d: null image", j);
        SLIME_REQUIRE(J.img_stride >= (long)J.img_w * 3, "view_jobs: job %d: row stride %ld smaller than a row of %d bytes", j, J.img_stride, J.img_w * 3);
        const int ks_h = slime_resample_ksize_ex(J.field_w, J.out_w, J.filter), ks_v = slime_resample_ksize_ex(J.field_h, J.out_h, J.filter);
        SLIME_REQUIRE(J.out_w == J.field_w || (J.bounds_h && J.kk_h && J.ksize_h == ks_h),
                      "view_jobs: job %d: horizontal tables missing or ksize %d != %d", j, J.ksize_h, ks_h);
        SLIME_REQUIRE(J.out_h == J.field_h || (J.bounds_v && J.kk_v && J.ksize_v == ks_v),
                      "view_jobs: job %d: vertical tables missing or ksize %d != %d", j, J.ksize_v, ks_v);
        const long wins = (long)J.win_nx * J.win_ny;
        SLIME_REQUIRE(J.first_crop >= 0 && J.first_crop <= out_crops && wins <= out_crops - J.first_crop,
                      "view_jobs: job %d: crops [%ld, %ld) outside the output's [0, %ld)", j, J.first_crop, J.first_crop + wins, out_crops);
        for (int i = 0; i < j; ++i) {
            const long wi = (long)jobs[i].win_nx * jobs[i].win_ny;
            SLIME_REQUIRE(J.first_crop >= jobs[i].first_crop + wi || jobs[i].first_crop >= J.first_crop + wins,
                          "view_jobs: crops of jobs %d and %d overlap ([%ld, %ld) and [%ld, %ld))", i, j, jobs[i].first_crop, jobs[i].first_crop + wi,
                          J.first_crop, J.first_crop + wins);
        }
        SLIME_REQUIRE(J.tmp_offset == p.tmp_offset[j] && J.h_block0 == p.h_block0[j] && J.v_block0 == p.v_block0[j],
                      "view_jobs: job %d: tmp_offset / h_block0 / v_block0 are not what slime_view_jobs_plan sets (plan not run?)", j);
    }
    if (p.tmp_bytes && (!tmp || tmp_bytes < p.tmp_bytes || ((size_t)tmp & 15))) {
        slime_set_error("view_jobs: tmp needs %zu bytes, 16-byte aligned (got %zu at %p)", p.tmp_bytes, tmp ? tmp_bytes : (size_t)0, (void*)tmp);
        return SLIME_EWORKSPACE;
    }
    if (p.h_blocks) {
        hipLaunchKernelGGL(view_h_kernel, dim3((unsigned)p.h_blocks), dim3(256), 0, (hipStream_t)stream, jobs_dev, n_jobs, crop, tmp);
        SLIME_CHECK_LAUNCH("view_h");
    }
    const float3 mean = make_float3(mean3[0], mean3[1], mean3[2]), sd = make_float3(std3[0], std3[1], std3[2]);
    const dim3 grid((unsigned)p.v_blocks), block(256);
    const size_t lds = align_up((size_t)crop * 3, 4);
    if (out_dtype == SLIME_F16) hipLaunchKernelGGL((view_v_kernel<F16>), grid, block, lds, (hipStream_t)stream, jobs_dev, n_jobs, crop, tmp, mean, sd, out, out_dtype);
    else hipLaunchKernelGGL((view_v_kernel<BF16>), grid, block, lds, (hipStream_t)stream, jobs_dev, n_jobs, crop, tmp, mean, sd, out, out_dtype);
    SLIME_CHECK_LAUNCH("view_v");
    return SLIME_OK;
}
