// router_attn.inc -- the ATTENTION text-guided router (mm_resampler_type = 'qformer': TextGuidedRouterAttention.forward,
// llava/model/multimodal_resampler/builder.py:149-162, eval path), included by router.hip.
//
// Per image, x [T, H] the merged local tokens, text [L, H], mask [L]:
//     xq = ln_q(x); tk = ln_kv(text[mask != 0])
//     q = xq Wq^T + bq; k | v = tk [Wk; Wv]^T + [bk; bv]                   (cross_attn.in_proj_weight rows [q; k; v])
//     ctx = softmax(q k^T / sqrt(128)) v per head                          (the masked keys were never gathered: no mask in the kernel)
//     y = ln_post(ctx Wo^T + bo);  logit = relu(y W1^T + b1) . w2 + b2;  scores = softmax(logit / temp) over the T tokens
// The matrix work goes through slime_gemm_ex and slime_attention as they are; the three kernels here are the row passes between
// them.  The selection that follows (a second softmax / temp, sort, top-p) is slime_router_select[_batched].

// ---- 1. gathered LayerNorm of any width: out[r] = T(LN(src[idx[r]])), fp32 rows in, compact T rows out ---------------------------
// One wave per row, the row in registers (NCH float4 per lane, chunk c = i * 64 + lane, predicated on c < D / 4 so that any
// D % 128 == 0 up to 256 * NCH fits an instantiation), two-pass variance, fp32 statistics, 16-byte loads, butterfly reductions.
// DEPTH OF THE SUMS: a lane adds its 4 * NCH values in turn, then six butterfly levels: L = 4 * ceil(D / 256) + 6.
// The mean and the variance divide by D with a correctly rounded division (D need not be a power of two: 5120).
// idx == NULL is the identity; an index outside [0, src_rows) reads nothing (its row is LN of zeros: the bias).
struct LnGatherArgs {
    const float* src; long src_rows; const long long* idx; int rows; int D;
    const float* w; const float* b; float eps; void* out;
};

template <typename T, int NCH>
__global__ void __launch_bounds__(256) ln_gather_kernel(LnGatherArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int nch = a.D >> 2;                              // float4 chunks of a row
    const long long s = a.idx ? a.idx[row] : (long long)row;
    const bool ok = s >= 0 && s < a.src_rows;
    const float4* xr = reinterpret_cast<const float4*>(a.src + (size_t)(ok ? s : 0) * a.D);
    float4 v[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = i * 64 + lane;
        v[i] = (ok && c < nch) ? xr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) sum += v[i].x + v[i].y + v[i].z + v[i].w;     // padding chunks add exact zeros
    const float fD = (float)a.D;
    const float mean = __fdiv_rn(wave_sum(sum), fD);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        if (i * 64 + lane < nch) {
            float d;
            d = __fsub_rn(v[i].x, mean); q = __fmaf_rn(d, d, q);
            d = __fsub_rn(v[i].y, mean); q = __fmaf_rn(d, d, q);
            d = __fsub_rn(v[i].z, mean); q = __fmaf_rn(d, d, q);
            d = __fsub_rn(v[i].w, mean); q = __fmaf_rn(d, d, q);
        }
    }
    const float rstd = rsqrtf(__fadd_rn(__fdiv_rn(wave_sum(q), fD), a.eps));
    char* o = reinterpret_cast<char*>(a.out) + (size_t)row * a.D * 2;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = i * 64 + lane;
        if (c < nch) {
            const float4 w = reinterpret_cast<const float4*>(a.w)[c], b = reinterpret_cast<const float4*>(a.b)[c];
            const float y0 = __fmaf_rn(__fmul_rn(__fsub_rn(v[i].x, mean), rstd), w.x, b.x);
            const float y1 = __fmaf_rn(__fmul_rn(__fsub_rn(v[i].y, mean), rstd), w.y, b.y);
            const float y2 = __fmaf_rn(__fmul_rn(__fsub_rn(v[i].z, mean), rstd), w.z, b.z);
            const float y3 = __fmaf_rn(__fmul_rn(__fsub_rn(v[i].w, mean), rstd), w.w, b.w);
            u32x2 p = {T::pack2(y0, y1), T::pack2(y2, y3)};
            *reinterpret_cast<u32x2*>(o + (size_t)c * 8) = p;
        }
    }
}

template <typename T>
static void launch_ln_gather_t(const LnGatherArgs& a, hipStream_t s) {
    const dim3 grid((a.rows + 3) / 4), block(256);
    const int need = (a.D + 255) / 256;
    if (need <= 1) hipLaunchKernelGGL((ln_gather_kernel<T, 1>), grid, block, 0, s, a);
    else if (need <= 2) hipLaunchKernelGGL((ln_gather_kernel<T, 2>), grid, block, 0, s, a);
    else if (need <= 4) hipLaunchKernelGGL((ln_gather_kernel<T, 4>), grid, block, 0, s, a);
    else if (need <= 8) hipLaunchKernelGGL((ln_gather_kernel<T, 8>), grid, block, 0, s, a);
    else if (need <= 16) hipLaunchKernelGGL((ln_gather_kernel<T, 16>), grid, block, 0, s, a);
    else if (need <= 20) hipLaunchKernelGGL((ln_gather_kernel<T, 20>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ln_gather_kernel<T, 32>), grid, block, 0, s, a);
}

#define ROUTER_ATTN_MAX_H 8192
static int ln_gather_check(const float* src, long src_rows, int rows, int D, const float* w, const float* b, const void* out, int dtype) {
    SLIME_REQUIRE(src && w && b && out, "ln_gather: null pointer");
    SLIME_REQUIRE(rows > 0 && src_rows > 0, "ln_gather: empty input (rows=%d, src_rows=%ld)", rows, src_rows);
    SLIME_REQUIRE(D % 128 == 0 && D >= 128 && D <= ROUTER_ATTN_MAX_H, "ln_gather: D=%d must be a multiple of 128 in 128..%d", D, ROUTER_ATTN_MAX_H);
    SLIME_REQUIRE(dtype == SLIME_BF16 || dtype == SLIME_F16, "ln_gather: dtype %d is not a 16-bit MFMA type", dtype);
    SLIME_REQUIRE(((uintptr_t)src | (uintptr_t)w | (uintptr_t)b | (uintptr_t)out) % 16 == 0, "ln_gather: pointers must be 16-byte aligned");
    return SLIME_OK;
}
static void ln_gather_launch(const float* src, long src_rows, const long long* idx, int rows, int D, const float* w, const float* b,
                             float eps, void* out, int dtype, hipStream_t s) {
    LnGatherArgs a{src, src_rows, idx, rows, D, w, b, eps, out};
    if (dtype == SLIME_F16) launch_ln_gather_t<F16>(a, s); else launch_ln_gather_t<BF16>(a, s);
}

extern "C" int slime_ln_gather(const float* src, long src_rows, const long long* idx, int rows, int D, const float* w, const float* b,
                               float eps, void* out_t, int dtype, void* stream) {
    if (int rc = ln_gather_check(src, src_rows, rows, D, w, b, out_t, dtype)) return rc;
    SLIME_REQUIRE(!idx || (uintptr_t)idx % 8 == 0, "ln_gather: idx must be 8-byte aligned");
    ln_gather_launch(src, src_rows, idx, rows, D, w, b, eps, out_t, dtype, (hipStream_t)stream);
    SLIME_CHECK_LAUNCH("ln_gather");
    return SLIME_OK;
}

// ---- 2. probability head: logit[r] = b2 + sum_j max(h[r, j], 0) * w2[j] over fp32 rows h [rows, N1], N1 % 128 == 0 ----------------
// One WAVE per row, four rows per workgroup: at N1 = 1024 a row is 4 KiB = four 16-byte loads per lane, the kernel holds a handful
// of registers (full occupancy), and the reduction is six shuffles -- a workgroup per row would give every thread one load and pay
// an LDS round and a barrier for the four partial sums.  Depth of the sum: N1 / 64 products per lane in turn (fma), six butterfly
// levels, then + b2.
__global__ void __launch_bounds__(256) router_prob_head_kernel(const float* h, const float* w2, float b2, float* logit, int rows, int N1) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float4* hr = reinterpret_cast<const float4*>(h + (size_t)row * N1);
    const float4* wr = reinterpret_cast<const float4*>(w2);
    float s = 0.f;
    for (int c = lane; c < (N1 >> 2); c += 64) {
        const float4 x = hr[c], w = wr[c];
        s = __fmaf_rn(fmaxf(x.x, 0.f), w.x, s); s = __fmaf_rn(fmaxf(x.y, 0.f), w.y, s);
        s = __fmaf_rn(fmaxf(x.z, 0.f), w.z, s); s = __fmaf_rn(fmaxf(x.w, 0.f), w.w, s);
    }
    s = wave_sum(s);
    if (lane == 0) logit[row] = __fadd_rn(s, b2);
}

// ---- 3. scores[i] = softmax(logit / temp)[i] over the n logits of one image (one workgroup; fp32, max-subtracted expf) -----------
// n <= ROUTER_MAX_T; entries of `scores` past n are not touched.
__global__ void __launch_bounds__(256) router_logit_softmax_kernel(const float* logit, int n, float temp, float* scores) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float mx = -INFINITY;
    for (int i = tid; i < n; i += 256) mx = fmaxf(mx, logit[i] / temp);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sm = 0.f;
    for (int i = tid; i < n; i += 256) sm += expf(logit[i] / temp - mx);
    sm = wave_sum(sm);
    if (lane == 0) red[wv] = sm;
    __syncthreads();
    sm = (red[0] + red[1]) + (red[2] + red[3]);
    for (int i = tid; i < n; i += 256) scores[i] = expf(logit[i] / temp - mx) / sm;
}

extern "C" int slime_router_prob_head(const float* h, int rows, int N1, const float* w2, float b2, const int* n_rows_host, int B, int T_max,
                                      float temp, float* logit, float* scores, void* stream) {
    SLIME_REQUIRE(h && w2 && logit, "router_prob_head: null pointer");
    SLIME_REQUIRE(rows > 0 && N1 > 0 && N1 % 128 == 0, "router_prob_head: rows=%d, N1=%d (a multiple of 128)", rows, N1);
    SLIME_REQUIRE(((uintptr_t)h | (uintptr_t)w2) % 16 == 0, "router_prob_head: pointers must be 16-byte aligned");
    if (scores) {
        SLIME_REQUIRE(n_rows_host && B > 0 && temp > 0.f, "router_prob_head: the softmax needs n_rows_host, B > 0 and a positive temperature");
        SLIME_REQUIRE(T_max > 0 && T_max <= ROUTER_MAX_T, "router_prob_head: T_max=%d outside 1..%d", T_max, ROUTER_MAX_T);
        long sum = 0;
        for (int b = 0; b < B; ++b) {
            SLIME_REQUIRE(n_rows_host[b] >= 0 && n_rows_host[b] <= T_max, "router_prob_head: n_rows[%d]=%d outside 0..T_max=%d", b, n_rows_host[b], T_max);
            sum += n_rows_host[b];
        }
        SLIME_REQUIRE(sum == rows, "router_prob_head: the segments cover %ld rows, not %d", sum, rows);
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(router_prob_head_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, h, w2, b2, logit, rows, N1);
    if (scores) {
        long off = 0;
        for (int b = 0; b < B; ++b) {
            if (n_rows_host[b] > 0)
                hipLaunchKernelGGL(router_logit_softmax_kernel, dim3(1), dim3(256), 0, s, logit + off, n_rows_host[b], temp, scores + (size_t)b * T_max);
            off += n_rows_host[b];
        }
    }
    SLIME_CHECK_LAUNCH("router_prob_head");
    return SLIME_OK;
}

// ---- the whole score path --------------------------------------------------------------------------------------------------------
struct RouterAttnPlan { size_t xq, tk, q, kv, ctx, o32, h, logit, total; };
#define ROUTER_ATTN_SLACK_ROWS 128      // rows behind every operand buffer: a tile edge of a GEMM / attention launch stays inside the workspace
static RouterAttnPlan router_attn_plan(const slime_router_attn_desc* d, long sum_T, long sum_L) {
    const size_t H = d->H, ST = (size_t)sum_T + ROUTER_ATTN_SLACK_ROWS, SL = (size_t)sum_L + ROUTER_ATTN_SLACK_ROWS;
    RouterAttnPlan p{};
    size_t off = 0;
    auto take = [&](size_t b) { size_t o = align_up(off, 256); off = o + b; return o; };
    p.xq = take(ST * H * 2);                     // ln_q(x), later ln_post(o32)
    p.tk = take(SL * H * 2);
    p.q = take(ST * H * 2);
    p.kv = take(SL * 2 * H * 2);
    p.ctx = take(ST * H * 2);
    p.o32 = take(ST * H * 4);
    p.h = take(ST * (size_t)d->N1 * 4);
    p.logit = take(ST * 4);
    p.total = align_up(off, 256);
    return p;
}

static int router_attn_validate(const slime_router_attn_desc* d) {
    SLIME_REQUIRE(d, "router_attn: null descriptor");
    SLIME_REQUIRE(d->dtype == SLIME_BF16 || d->dtype == SLIME_F16, "router_attn: dtype must be BF16 or F16");
    SLIME_REQUIRE(d->H >= 128 && d->H % 128 == 0, "router_attn: H=%d must be a positive multiple of 128 (head_dim 128)", d->H);
    SLIME_REQUIRE(d->H <= ROUTER_ATTN_MAX_H, "router_attn: H=%d exceeds %d", d->H, ROUTER_ATTN_MAX_H);
    SLIME_REQUIRE(d->heads * 128 == d->H, "router_attn: heads=%d must be H / 128 = %d", d->heads, d->H / 128);
    SLIME_REQUIRE(d->N1 > 0 && d->N1 % 128 == 0, "router_attn: N1=%d must be H / 4 padded to a multiple of 128", d->N1);
    SLIME_REQUIRE(d->ln_q_w && d->ln_q_b && d->ln_kv_w && d->ln_kv_b && d->ln_post_w && d->ln_post_b && (d->w_q || d->w_q_frag) && d->b_q &&
                  (d->w_kv || d->w_kv_frag) && d->b_kv && (d->w_o || d->w_o_frag) && d->b_o && (d->w_1 || d->w_1_frag) && d->b_1 && d->w_2,
                  "router_attn: missing weights");
    SLIME_REQUIRE(((uintptr_t)d->ln_q_w | (uintptr_t)d->ln_q_b | (uintptr_t)d->ln_kv_w | (uintptr_t)d->ln_kv_b | (uintptr_t)d->ln_post_w |
                   (uintptr_t)d->ln_post_b | (uintptr_t)d->w_q | (uintptr_t)d->b_q | (uintptr_t)d->w_kv | (uintptr_t)d->b_kv | (uintptr_t)d->w_o |
                   (uintptr_t)d->b_o | (uintptr_t)d->w_1 | (uintptr_t)d->b_1 | (uintptr_t)d->w_2 | (uintptr_t)d->w_q_frag | (uintptr_t)d->w_kv_frag |
                   (uintptr_t)d->w_o_frag | (uintptr_t)d->w_1_frag) % 16 == 0, "router_attn: weight pointers must be 16-byte aligned");
    return SLIME_OK;
}

extern "C" size_t slime_router_attn_workspace_bytes(const slime_router_attn_desc* d, long sum_T, long sum_L) {
    if (!d || sum_T <= 0 || sum_L <= 0 || d->H <= 0 || d->N1 <= 0) return 0;
    return router_attn_plan(d, sum_T, sum_L).total;
}

static int router_attn_gemm(const void* A, const void* B, const void* B_frag, const float* bias, void* C, int M, int N, int K, int dtype,
                            int epilogue, void* stream) {
    slime_gemm_args g{};
    g.A = A; g.lda = K; g.B = B; g.B_frag = B_frag; g.bias = bias; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K; g.dtype = dtype; g.epilogue = epilogue;
    return slime_gemm_ex(&g, stream);
}

extern "C" int slime_router_attn_scores(const slime_router_attn_desc* d, const float* tokens, long token_rows, const long long* tok_idx,
                                        const int* n_rows_host, const float* text, long text_rows, const long long* key_idx,
                                        const int* n_keys_host, int B, int T_max, float temp, float* scores, void* ws, size_t ws_bytes,
                                        void* stream) {
    // every check precedes the first launch
    if (int rc = router_attn_validate(d)) return rc;
    SLIME_REQUIRE(tokens && tok_idx && n_rows_host && text && key_idx && n_keys_host && scores, "router_attn_scores: null pointer");
    SLIME_REQUIRE(B > 0 && token_rows > 0 && text_rows > 0, "router_attn_scores: empty batch (B=%d, token_rows=%ld, text_rows=%ld)", B, token_rows, text_rows);
    SLIME_REQUIRE(T_max > 0 && T_max <= ROUTER_MAX_T, "router_attn_scores: T_max=%d outside 1..%d (the select kernel's limit)", T_max, ROUTER_MAX_T);
    SLIME_REQUIRE(temp > 0.f, "router_attn_scores: temperature must be positive");
    SLIME_REQUIRE(((uintptr_t)tokens | (uintptr_t)text) % 16 == 0 && ((uintptr_t)tok_idx | (uintptr_t)key_idx) % 8 == 0 && (uintptr_t)scores % 4 == 0,
                  "router_attn_scores: tokens / text must be 16-byte, the index arrays 8-byte and scores 4-byte aligned");
    long sum_T = 0, sum_L = 0;
    for (int b = 0; b < B; ++b) {
        SLIME_REQUIRE(n_rows_host[b] >= 0 && n_rows_host[b] <= T_max, "router_attn_scores: n_rows[%d]=%d outside 0..T_max=%d", b, n_rows_host[b], T_max);
        SLIME_REQUIRE(n_keys_host[b] >= 0, "router_attn_scores: n_keys[%d]=%d is negative", b, n_keys_host[b]);
        SLIME_REQUIRE(n_rows_host[b] == 0 || n_keys_host[b] > 0,
                      "router_attn_scores: image %d has %d tokens and no valid text key (the softmax over the keys is undefined)", b, n_rows_host[b]);
        sum_T += n_rows_host[b];
        if (n_rows_host[b] > 0) sum_L += n_keys_host[b];
    }
    SLIME_REQUIRE(sum_T < (1L << 31) / 2 && sum_L < (1L << 31) / 2, "router_attn_scores: %ld token rows / %ld keys exceed 2^30", sum_T, sum_L);
    if (sum_T == 0) return SLIME_OK;                                    // nothing to score: no launch
    const RouterAttnPlan p = router_attn_plan(d, sum_T, sum_L);
    if (!ws || ws_bytes < p.total || ((uintptr_t)ws % 256) != 0) {
        slime_set_error("router_attn_scores: workspace %zu B (need %zu, 256-B aligned)", ws_bytes, p.total);
        return SLIME_EWORKSPACE;
    }
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    const int H = d->H, N1 = d->N1, dt = d->dtype, ST = (int)sum_T, SL = (int)sum_L;
    // key_idx lists the valid keys of the images WITH tokens, image after image (an image without tokens contributes none)
    ln_gather_launch(tokens, token_rows, tok_idx, ST, H, d->ln_q_w, d->ln_q_b, d->eps, w + p.xq, dt, s);
    ln_gather_launch(text, text_rows, key_idx, SL, H, d->ln_kv_w, d->ln_kv_b, d->eps, w + p.tk, dt, s);
    SLIME_CHECK_LAUNCH("router_attn_scores (ln_gather)");
    if (int rc = router_attn_gemm(w + p.xq, d->w_q, d->w_q_frag, d->b_q, w + p.q, ST, H, H, dt, SLIME_EPI_BIAS_T, stream)) return rc;
    if (int rc = router_attn_gemm(w + p.tk, d->w_kv, d->w_kv_frag, d->b_kv, w + p.kv, SL, 2 * H, H, dt, SLIME_EPI_BIAS_T, stream)) return rc;
    long t0 = 0, l0 = 0;
    for (int b = 0; b < B; ++b) {
        const int Tb = n_rows_host[b], Lb = n_keys_host[b];
        if (Tb == 0) continue;
        const char* kb = w + p.kv + (size_t)l0 * 2 * H * 2;
        if (int rc = slime_attention(w + p.q + (size_t)t0 * H * 2, 0, H, kb, 0, 2L * H, kb + (size_t)H * 2, 0, 2L * H,
                                     w + p.ctx + (size_t)t0 * H * 2, 0, H, 1, d->heads, 128, Tb, Lb, dt, stream)) return rc;
        t0 += Tb; l0 += Lb;
    }
    if (int rc = router_attn_gemm(w + p.ctx, d->w_o, d->w_o_frag, d->b_o, w + p.o32, ST, H, H, dt, SLIME_EPI_BIAS_F32, stream)) return rc;
    ln_gather_launch((const float*)(w + p.o32), ST, nullptr, ST, H, d->ln_post_w, d->ln_post_b, d->eps, w + p.xq, dt, s);
    SLIME_CHECK_LAUNCH("router_attn_scores (ln_post)");
    if (int rc = router_attn_gemm(w + p.xq, d->w_1, d->w_1_frag, d->b_1, w + p.h, ST, N1, H, dt, SLIME_EPI_BIAS_F32, stream)) return rc;
    return slime_router_prob_head((const float*)(w + p.h), ST, N1, d->w_2, d->b_2, n_rows_host, B, T_max, temp, (float*)(w + p.logit), scores, stream);
}
