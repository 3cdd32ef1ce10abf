// api.hip -- C-ABI drivers of libslime_hip: the CLIP tower layer loop, the Resampler, the projector
// MLP and the GatedBlock, each a fixed sequence of the primitive kernels on one stream.  No
// allocation, no synchronisation, no global mutable state (the last-error string is thread-local): callable under
// hipGraph capture.
#include <stdarg.h>
#include <string.h>
#include "common.h"
#include "adapter_ragged.h"

static thread_local char g_err[512] = "";

void slime_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* slime_last_error(void) { return g_err; }
// slime_gemm with the optional fragment-order copy of the static operand
static int gemm_w(const void* A, int lda, const void* B, const void* B_frag, const float* bias, void* C, int ldc, int M, int N, int K,
                  int dtype, int epilogue, void* stream) {
    slime_gemm_args a{};
    a.A = A; a.lda = lda; a.B = B; a.bias = bias; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.dtype = dtype; a.epilogue = epilogue;
    a.B_frag = B_frag;
    return slime_gemm_ex(&a, stream);
}

// projection[0] + GELU of both experts' rows and their gate mix in ONE launch (SLIME_EPI_BIAS_GELU_MIX_T; direct-B kernel only)
static bool mix_in_gemm(const slime_mlp_desc* m) {
    return m->w1_frag && m->hidden % 256 == 0 && m->in_dim % 64 == 0 && ((uintptr_t)m->w1_frag % 16) == 0;
}
static int gemm_mix(const void* A, const void* A2, const float* gates, const slime_mlp_desc* m, void* C, int tokens, void* stream) {
    slime_gemm_args a{};
    a.A = A; a.A2 = A2; a.mix_gates = gates; a.lda = m->in_dim; a.B = m->w1; a.B_frag = m->w1_frag; a.bias = m->b1; a.C = C; a.ldc = m->hidden;
    a.M = tokens; a.N = m->hidden; a.K = m->in_dim; a.dtype = m->dtype; a.epilogue = SLIME_EPI_BIAS_GELU_MIX_T;
    return slime_gemm_ex(&a, stream);
}

extern "C" int slime_abi_version(void) { return SLIME_ABI_VERSION; }

#define TRY(call)                     \
    do {                              \
        int rc_ = (call);             \
        if (rc_ != SLIME_OK) return rc_; \
    } while (0)

namespace {
static bool is16(int dt) { return dt == SLIME_BF16 || dt == SLIME_F16; }
}  // namespace

// every driver's workspace: `need` bytes at a 256-B aligned address
static int ws_check(const char* name, const void* ws, size_t ws_bytes, size_t need) {
    if (ws && ws_bytes >= need && ((uintptr_t)ws % 256) == 0) return SLIME_OK;
    slime_set_error("%s: workspace %zu B (need %zu, 256-B aligned)", name, ws_bytes, need);
    return SLIME_EWORKSPACE;
}

// ------------------------------------------------------------------------------------------------
// CLIP tower
// ------------------------------------------------------------------------------------------------
// Round 5: the residual stream between the layers is SPLIT (hi = T(h), which IS the next GEMM's operand, + a lower part) instead of
// fp32 rows plus a separate T(h) copy; round 6 (ABI 7): the lower part is one signed byte per element (common.h resid_delta): the
// out_proj / fc2 epilogues (SLIME_EPI_BIAS_RESID_SPLIT_LN) move 6 bytes per element -- 8 with a 16-bit lower part (round 5), 10 with
// the fp32 stream of rounds 1-4.
struct VitPlan {
    size_t xn, qkv, ctx, ff, lo, stats, total;  // offsets (lo: the lower part of the split stream, one byte per element)
};

// The three tower forms the layer loop serves (vit_run): the CLIP layout (class token + pre-LayerNorm, S = P + 1 rows per crop), the
// plain one of the SigLIP towers (S = P rows behind slime_patch_embed_plain, fc1 with the tanh-form GELU) and the prefix one of the
// DINOv2 towers (n_prefix > 0: S = n_prefix + P rows behind slime_patch_embed_prefix, no pre-LayerNorm, fc1 with the exact GELU).
// `lead` = the rows in front of a crop's patches: the class token, none, the n_prefix table rows.
struct VitForm { bool plain; int fc1_epilogue; int n_prefix; int lead; };
static VitForm clip_form(int act = SLIME_ACT_QUICKGELU) {
    return {false, act == SLIME_ACT_GELU ? SLIME_EPI_BIAS_GELU_T : SLIME_EPI_BIAS_QUICKGELU_T, 0, 1};
}
static VitForm siglip_form() { return {true, SLIME_EPI_BIAS_GELU_TANH_T, 0, 0}; }
static VitForm dinov2_form(int n_prefix) { return {false, SLIME_EPI_BIAS_GELU_T, n_prefix, n_prefix}; }

static int vit_seq(const slime_vit_desc* d, const VitForm& form) {
    const int g = d->image / d->patch;
    return g * g + form.lead;
}

static VitPlan vit_plan(const slime_vit_desc* d, int n, const VitForm& form) {
    const int S = vit_seq(d, form);
    const size_t M = (size_t)n * S, D = d->hidden;
    VitPlan p{};
    size_t off = 0;
    auto take = [&](size_t b) { size_t o = align_up(off, 256); off = o + b; return o; };
    p.lo = take(M * D);
    p.xn = take(M * D * 2);
    const size_t ff_bytes = M * (size_t)d->inter * 2;
    // q/k/v and the attention context die before fc1 writes the MLP's intermediate rows, and those die before the next layer's q/k/v
    // GEMM: the three share one region (for CLIP-L, 3 D + D = the intermediate width exactly).  The launches of a stream are serial, so
    // nothing else changes -- except that a 20-crop stream now cycles through 165 MB instead of 260, and the 256 MiB memory-side
    // cache, which two such streams share, keeps more of what the next kernel reads (profiles/r04_fabric_traffic.txt).
    const size_t qkv_bytes = align_up(M * 3 * D * 2, 256), attn_bytes = qkv_bytes + M * D * 2;
    const size_t region = ff_bytes > attn_bytes ? ff_bytes : attn_bytes;
    p.ff = take(region);
    p.qkv = p.ff;
    p.ctx = p.ff + qkv_bytes;
    p.stats = take(M * (D / 64) * 2 * sizeof(float));      // LayerNorm fold: (sum, sum of squares) per row and 64-column group
    p.total = align_up(off, 256);
    return p;
}

int slime_patch_embed_geometry(int image, int patch, int kpad, int D, size_t* lds_out);   // patch_embed.hip: the fused front end's limits

static int vit_validate(const slime_vit_desc* d, const VitForm& form) {
    SLIME_REQUIRE(d, "vit: null descriptor");
    if (form.n_prefix > 0) {                             // the DINOv2 entries: cls carries the prefix table, the pre-LayerNorm fields stay empty
        SLIME_REQUIRE(d->cls, "dinov2: cls is required (the prefix table [n_prefix, hidden]: class token + position 0, then the register tokens)");
        SLIME_REQUIRE(!d->pre_ln_w, "dinov2: pre_ln_w must be NULL (a DINOv2 tower has no pre-LayerNorm)");
        SLIME_REQUIRE(!d->pre_ln_b, "dinov2: pre_ln_b must be NULL (a DINOv2 tower has no pre-LayerNorm)");
    } else if (form.plain) {                                    // the SigLIP entries: the descriptor's class-token / pre-LayerNorm fields stay empty
        SLIME_REQUIRE(!d->cls, "siglip: cls must be NULL (a SigLIP tower has no class token; slime_vit_forward* run the CLIP layout)");
        SLIME_REQUIRE(!d->pre_ln_w, "siglip: pre_ln_w must be NULL (a SigLIP tower has no pre-LayerNorm)");
        SLIME_REQUIRE(!d->pre_ln_b, "siglip: pre_ln_b must be NULL (a SigLIP tower has no pre-LayerNorm)");
    }
    SLIME_REQUIRE(is16(d->dtype), "vit: dtype must be BF16 or F16");
    SLIME_REQUIRE(d->hidden == 128 || d->hidden == 256 || d->hidden == 768 || d->hidden == 1024, "vit: hidden=%d unsupported", d->hidden);
    SLIME_REQUIRE(d->hidden % 64 == 0, "vit: hidden must be a multiple of 64 (LayerNorm partial sums per 64 columns)");
    SLIME_REQUIRE(d->heads > 0 && d->hidden % d->heads == 0 && d->hidden / d->heads == 64, "vit: head_dim must be 64");
    SLIME_REQUIRE(d->inter % 128 == 0 && d->inter % 64 == 0, "vit: intermediate size %d must be a multiple of 128", d->inter);
    SLIME_REQUIRE(d->patch > 0 && d->image % d->patch == 0, "vit: image %d not a multiple of patch %d", d->image, d->patch);
    TRY(slime_patch_embed_geometry(d->image, d->patch, d->kpad, d->hidden, nullptr));      // the one-launch front end's geometry limits
    SLIME_REQUIRE(d->layers_run >= 0, "vit: layers_run < 0");
    SLIME_REQUIRE(d->patch_w_frag && d->pos && (form.plain || form.n_prefix > 0 || (d->cls && d->pre_ln_w && d->pre_ln_b)),
                  "vit: missing embedding weights (patch_w_frag = slime_gemm_pack_b of the conv weight is required since ABI 5)");
    // a per-layer weight is given as its fragment-order image, its row-major image, or both (slime_gemm_b_frag_usable)
    SLIME_REQUIRE(d->layers_run == 0 || ((d->w_qkv || d->w_qkv_frag) && d->b_qkv && d->colsum_qkv && (d->w_o || d->w_o_frag) && d->b_o &&
                                         (d->w_fc1 || d->w_fc1_frag) && d->b_fc1 && d->colsum_fc1 && (d->w_fc2 || d->w_fc2_frag) && d->b_fc2),
                  "vit: missing layer weights");
    return SLIME_OK;
}

// splits per layer GEMM (slime_vit_forward_ksplit): each within its GEMM's range -- 1..SLIME_GEMM_KSPLIT_MAX and at most K / 64
static int vit_ksplit_validate(const slime_vit_desc* d, const slime_vit_ksplit* ks) {
    const int kmax_d = d->hidden / 64 < SLIME_GEMM_KSPLIT_MAX ? d->hidden / 64 : SLIME_GEMM_KSPLIT_MAX;
    const int kmax_f = d->inter / 64 < SLIME_GEMM_KSPLIT_MAX ? d->inter / 64 : SLIME_GEMM_KSPLIT_MAX;
    SLIME_REQUIRE(ks->qkv >= 1 && ks->qkv <= kmax_d, "vit: k-split qkv=%d outside 1..%d (K = hidden = %d)", ks->qkv, kmax_d, d->hidden);
    SLIME_REQUIRE(ks->out_proj >= 1 && ks->out_proj <= kmax_d, "vit: k-split out_proj=%d outside 1..%d (K = hidden = %d)", ks->out_proj, kmax_d, d->hidden);
    SLIME_REQUIRE(ks->fc1 >= 1 && ks->fc1 <= kmax_d, "vit: k-split fc1=%d outside 1..%d (K = hidden = %d)", ks->fc1, kmax_d, d->hidden);
    SLIME_REQUIRE(ks->fc2 >= 1 && ks->fc2 <= kmax_f, "vit: k-split fc2=%d outside 1..%d (K = intermediate = %d)", ks->fc2, kmax_f, d->inter);
    return SLIME_OK;
}

static size_t vit_ksplit_partial_bytes(const slime_vit_desc* d, int n, const slime_vit_ksplit* ks, const VitForm& form) {
    const int M = n * vit_seq(d, form);
    size_t b = slime_gemm_ksplit_workspace_bytes(M, 3 * d->hidden, ks->qkv);
    auto grow = [&](size_t x) { if (x > b) b = x; };
    grow(slime_gemm_ksplit_workspace_bytes(M, d->hidden, ks->out_proj));
    grow(slime_gemm_ksplit_workspace_bytes(M, d->inter, ks->fc1));
    grow(slime_gemm_ksplit_workspace_bytes(M, d->hidden, ks->fc2));
    return b;
}

// diagnostic build only (libslime_hip_diag.so; results become wrong): bit k set = the tower skips kernel id k of every layer, to read each kernel's
// MARGINAL cost inside the two-stream tower (tools/marginal_bench.py)
#ifdef SLIME_DIAG
static int g_vit_skip_mask = 0;
extern "C" void slime_vit_set_skip_mask(int m) { g_vit_skip_mask = m; }
#else
static constexpr int g_vit_skip_mask = 0;
#endif

#define PROBED(kid, call)                                                                             \
    do {                                                                                              \
        const bool on_ = probe && probe->layer == l && probe->kernel == (kid);                        \
        if (on_ && probe->start) (void)hipEventRecord((hipEvent_t)probe->start, (hipStream_t)stream);       \
        if (!((g_vit_skip_mask >> (kid)) & 1)) TRY(call);                                             \
        if (on_ && probe->stop) (void)hipEventRecord((hipEvent_t)probe->stop, (hipStream_t)stream);          \
    } while (0)

static int vit_run(const slime_vit_desc* d, const void* pixels, int pix_dtype, int n, void* out, int out_dtype, int keep_cls,
                   float* hidden_f32, void* ws, size_t ws_bytes, void* stream, const slime_probe* probe, float* states,
                   const slime_vit_ksplit* ks, const VitForm& form) {
    TRY(vit_validate(d, form));
    SLIME_REQUIRE(pixels && n > 0, "vit: bad input");
    SLIME_REQUIRE(out || hidden_f32 || states, "vit: no output requested");
    SLIME_REQUIRE(!out || out_dtype == SLIME_F32 || is16(out_dtype), "vit: bad out dtype");
    if (ks) TRY(vit_ksplit_validate(d, ks));
    const VitPlan p = vit_plan(d, n, form);
    const size_t part_bytes = ks ? vit_ksplit_partial_bytes(d, n, ks, form) : 0;      // one region of partial products behind the plan
    TRY(ws_check("vit", ws, ws_bytes, p.total + part_bytes));
    // a layer GEMM: slime_gemm_ex, or the split pair where the caller asked for one (the probe brackets the GEMM as a whole)
    auto layer_gemm = [&](const slime_gemm_args& a, int splits) {
        return splits > 1 ? slime_gemm_ksplit(&a, splits, (char*)ws + p.total, part_bytes, stream) : slime_gemm_ex(&a, stream);
    };
    const slime_vit_ksplit k1{1, 1, 1, 1};
    const slime_vit_ksplit& sp = ks ? *ks : k1;
    const int S = vit_seq(d, form), lead = form.lead;
    const int P = S - lead, D = d->hidden, F = d->inter;
    const int M = n * S;
    char* w = (char*)ws;
    void* xn = w + p.xn;
    char* qkv = w + p.qkv;
    void* ctx = w + p.ctx;
    void* ff = w + p.ff;
    const int dt = d->dtype;
    float* stats = (float*)(w + p.stats);
    const int G = D / 64;
    // residual stream = (xn, lo): xn = T(h) is the upper part AND the operand of the q/k/v / fc1 GEMMs, lo = one signed byte per element (common.h resid_delta)
    void* lo = w + p.lo;

    // patch embed (MFMA conv), class token, position table, pre-LayerNorm and the first folded LN1's operand + partial sums: ONE launch
    // (no fp32 rows: h = NULL)
    // -- or, in the plain form, patch embed + position table alone (slime_patch_embed_plain: S = P rows per crop)
    // -- or, in the prefix form, the same behind n_prefix table rows (slime_patch_embed_prefix: S = n_prefix + P rows per crop)
    if (form.n_prefix > 0)
        TRY(slime_patch_embed_prefix(pixels, pix_dtype, d->patch_w_frag, d->cls, form.n_prefix, d->pos, nullptr, xn, lo, stats, dt, n, d->image,
                                     d->patch, d->kpad, D, stream));
    else if (form.plain)
        TRY(slime_patch_embed_plain(pixels, pix_dtype, d->patch_w_frag, d->pos, nullptr, xn, lo, stats, dt, n, d->image, d->patch, d->kpad, D,
                                    stream));
    else
        TRY(slime_patch_embed_prenorm(pixels, pix_dtype, d->patch_w_frag, d->cls, d->pos, d->pre_ln_w, d->pre_ln_b, d->eps, nullptr, xn, lo,
                                      stats, dt, n, d->image, d->patch, d->kpad, D, stream));
    // hidden_states[i] of HF's output_hidden_states=True (entry 0 = the pre-LayerNorm'd embeddings, entry i = after layer i):
    // the residual stream joined to fp32 on the call's stream (capturable), one per state
    auto snapshot = [&](int idx) { return slime_gather_rows_split(xn, lo, dt, S, 0, states + (size_t)idx * M * D, SLIME_F32, n, S, D, stream); };
    if (states) TRY(snapshot(0));

    // Layer loop, 5 launches per layer.  Both LayerNorms are FOLDED into the GEMMs around them (slime_gemm_ex): the GEMM that
    // updates the residual stream (previous fc2 / out_proj, or the embedding kernel) leaves the rows rounded to T (`xn`) and
    // their partial sums (`stats`); the q/k/v and fc1 GEMMs run on those un-normalised rows with gamma folded into their
    // weights and apply mean / rstd in the epilogue.  No LayerNorm kernel, no fp32 re-read of the residual stream.
    for (int l = 0; l < d->layers_run; ++l) {
        auto layer_w = [&](const void* base, size_t per_layer) -> const void* {     // this layer's slice of a per-layer weight (or NULL)
            return base ? (const char*)base + (size_t)l * per_layer * 2 : nullptr;
        };
        slime_gemm_args ga{};
        ga.M = M; ga.dtype = dt; ga.ln_eps = d->eps;
        // q/k/v = LN1(h) Wqkv^T + b  (HF :370-371, :309-311)
        ga.A = xn; ga.lda = D; ga.B = layer_w(d->w_qkv, (size_t)3 * D * D); ga.bias = d->b_qkv + (size_t)l * 3 * D; ga.C = qkv; ga.ldc = 3 * D;
        ga.N = 3 * D; ga.K = D;
        ga.epilogue = SLIME_EPI_BIAS_T; ga.ln_stats = stats; ga.ln_groups = G; ga.ln_colsum = d->colsum_qkv + (size_t)l * 3 * D;
        ga.B_frag = layer_w(d->w_qkv_frag, (size_t)3 * D * D);
        PROBED(1, layer_gemm(ga, sp.qkv));
        PROBED(2, slime_attention(qkv, (long)S * 3 * D, 3 * D, qkv + (size_t)D * 2, (long)S * 3 * D, 3 * D,
                                  qkv + (size_t)2 * D * 2, (long)S * 3 * D, 3 * D, ctx, (long)S * D, D, n, d->heads, 64, S, S,
                                  dt, stream));
        // the two GEMMs that update the residual stream and prepare the next folded LayerNorm (the last layer's partial sums are
        // written and never read)
        auto resid_update = [&](slime_gemm_args& r) {
            r.C = xn; r.ldc = D; r.lo8 = lo; r.ldlo = D; r.stats_out = stats; r.epilogue = SLIME_EPI_BIAS_RESID_SPLIT_LN;
        };
        // h += ctx Wo^T + b; leaves T(h) and its partial sums for LN2  (HF :372-377)
        ga = slime_gemm_args{};
        ga.M = M; ga.dtype = dt;
        ga.A = ctx; ga.lda = D; ga.B = layer_w(d->w_o, (size_t)D * D); ga.bias = d->b_o + (size_t)l * D; ga.N = D; ga.K = D;
        resid_update(ga);
        ga.B_frag = layer_w(d->w_o_frag, (size_t)D * D);
        PROBED(3, layer_gemm(ga, sp.out_proj));
        // ff = act(LN2(h) W1^T + b), act = quick_gelu, the erf GELU of the OpenCLIP towers or the tanh GELU of the SigLIP towers  (HF :379-380, :346-350)
        ga = slime_gemm_args{};
        ga.M = M; ga.dtype = dt; ga.ln_eps = d->eps;
        ga.A = xn; ga.lda = D; ga.B = layer_w(d->w_fc1, (size_t)F * D); ga.bias = d->b_fc1 + (size_t)l * F; ga.C = ff; ga.ldc = F; ga.N = F; ga.K = D;
        ga.epilogue = form.fc1_epilogue; ga.ln_stats = stats; ga.ln_groups = G; ga.ln_colsum = d->colsum_fc1 + (size_t)l * F;
        ga.B_frag = layer_w(d->w_fc1_frag, (size_t)F * D);
        PROBED(5, layer_gemm(ga, sp.fc1));
        // h += ff W2^T + b; prepares the next layer's LN1  (HF :381-383)
        ga = slime_gemm_args{};
        ga.M = M; ga.dtype = dt;
        ga.A = ff; ga.lda = F; ga.B = layer_w(d->w_fc2, (size_t)D * F); ga.bias = d->b_fc2 + (size_t)l * D; ga.N = D; ga.K = F;
        resid_update(ga);
        ga.B_frag = layer_w(d->w_fc2_frag, (size_t)D * F);
        PROBED(6, layer_gemm(ga, sp.fc2));
        if (states) TRY(snapshot(l + 1));
    }
    if (hidden_f32) TRY(slime_gather_rows_split(xn, lo, dt, S, 0, hidden_f32, SLIME_F32, n, S, D, stream));
    if (out) {
        // feature_select: 'patch' drops the class token (clip_encoder.py:38-39), cast to out dtype (:52,56); the plain form has none
        // (lead = 0: all S = P rows either way); the prefix form drops its n_prefix rows (keep_prefix = 0) or none
        TRY(slime_gather_rows_split(xn, lo, dt, S, keep_cls ? 0 : lead, out, out_dtype, n, keep_cls ? S : P, D, stream));
    }
    return SLIME_OK;
}

// what the six *_workspace_bytes entries return: the plan, plus the region of partial products where the pass is split (ks)
static size_t vit_workspace(const slime_vit_desc* d, int n_crops, const slime_vit_ksplit* ks, const VitForm& form) {
    if (!d || n_crops <= 0 || d->patch <= 0) return 0;
    return vit_plan(d, n_crops, form).total + (ks ? vit_ksplit_partial_bytes(d, n_crops, ks, form) : 0);
}

extern "C" int slime_vit_check(const slime_vit_desc* d) { return vit_validate(d, clip_form()); }

extern "C" int slime_vit_residual_epilogue(void) { return SLIME_EPI_BIAS_RESID_SPLIT_LN; }

extern "C" size_t slime_vit_workspace_bytes(const slime_vit_desc* d, int n_crops) { return vit_workspace(d, n_crops, nullptr, clip_form()); }

extern "C" int slime_vit_forward(const slime_vit_desc* d, const void* pixels, int pix_dtype, int n, void* out,
                                 int out_dtype, int keep_cls, float* hidden_f32, void* ws, size_t ws_bytes,
                                 void* stream) {
    return slime_vit_forward_ex(d, pixels, pix_dtype, n, out, out_dtype, keep_cls, hidden_f32, ws, ws_bytes, stream, nullptr);
}

extern "C" int slime_vit_forward_ex(const slime_vit_desc* d, const void* pixels, int pix_dtype, int n, void* out,
                                    int out_dtype, int keep_cls, float* hidden_f32, void* ws, size_t ws_bytes,
                                    void* stream, const slime_probe* probe) {
    return vit_run(d, pixels, pix_dtype, n, out, out_dtype, keep_cls, hidden_f32, ws, ws_bytes, stream, probe, nullptr, nullptr, clip_form());
}

extern "C" size_t slime_vit_ksplit_workspace_bytes(const slime_vit_desc* d, int n_crops, const slime_vit_ksplit* ks) {
    return ks ? vit_workspace(d, n_crops, ks, clip_form()) : 0;
}

extern "C" int slime_vit_forward_ksplit(const slime_vit_desc* d, const void* pixels, int pix_dtype, int n, void* out, int out_dtype,
                                        int keep_cls, float* hidden_f32, const slime_vit_ksplit* ks, void* ws, size_t ws_bytes, void* stream) {
    SLIME_REQUIRE(ks, "vit_forward_ksplit: null k-split setting (slime_vit_forward is the unsplit call)");
    return vit_run(d, pixels, pix_dtype, n, out, out_dtype, keep_cls, hidden_f32, ws, ws_bytes, stream, nullptr, nullptr, ks, clip_form());
}

extern "C" int slime_vit_forward_states(const slime_vit_desc* d, const void* pixels, int pix_dtype, int n, float* states_f32,
                                        void* ws, size_t ws_bytes, void* stream) {
    SLIME_REQUIRE(states_f32, "vit_forward_states: states_f32 is required");
    return vit_run(d, pixels, pix_dtype, n, nullptr, SLIME_F32, 1, nullptr, ws, ws_bytes, stream, nullptr, states_f32, nullptr, clip_form());
}

// The superset of slime_vit_forward / _ksplit / _states, with the options a descriptor does not carry (the MLP's activation).
extern "C" int slime_vit_forward_opts(const slime_vit_desc* d, const slime_vit_opts* opts, const void* pixels, int pix_dtype, int n,
                                      void* out, int out_dtype, int keep_cls, float* hidden_f32, float* states_f32,
                                      const slime_vit_ksplit* ks, void* ws, size_t ws_bytes, void* stream) {
    const int act = opts ? opts->act : SLIME_ACT_QUICKGELU;
    SLIME_REQUIRE(act == SLIME_ACT_QUICKGELU || act == SLIME_ACT_GELU, "vit_forward_opts: act=%d is neither SLIME_ACT_QUICKGELU (0) nor "
                                                                       "SLIME_ACT_GELU (1)", act);
    return vit_run(d, pixels, pix_dtype, n, out, out_dtype, keep_cls, hidden_f32, ws, ws_bytes, stream, nullptr, states_f32, ks,
                   clip_form(act));
}

// SigLIP towers: vit_run's layer loop in its plain form (include/slime_hip.h)
extern "C" int slime_siglip_check(const slime_vit_desc* d) { return vit_validate(d, siglip_form()); }

extern "C" size_t slime_siglip_workspace_bytes(const slime_vit_desc* d, int n_crops) { return vit_workspace(d, n_crops, nullptr, siglip_form()); }

extern "C" size_t slime_siglip_ksplit_workspace_bytes(const slime_vit_desc* d, int n_crops, const slime_vit_ksplit* ks) {
    return ks ? vit_workspace(d, n_crops, ks, siglip_form()) : 0;
}

extern "C" int slime_siglip_forward(const slime_vit_desc* d, const void* pixels, int pix_dtype, int n, void* out, int out_dtype,
                                    float* hidden_f32, float* states_f32, const slime_vit_ksplit* ks, void* ws, size_t ws_bytes,
                                    void* stream) {
    return vit_run(d, pixels, pix_dtype, n, out, out_dtype, 1, hidden_f32, ws, ws_bytes, stream, nullptr, states_f32, ks,
                   siglip_form());
}

// DINOv2 towers: vit_run's layer loop in its prefix form (include/slime_hip.h)
static int dinov2_prefix_ok(int n_prefix) {
    SLIME_REQUIRE(n_prefix >= 1 && n_prefix <= 17, "dinov2: n_prefix=%d outside 1..17 (the class token and at most 16 register tokens)", n_prefix);
    return SLIME_OK;
}

extern "C" int slime_dinov2_check(const slime_vit_desc* d, int n_prefix) {
    TRY(dinov2_prefix_ok(n_prefix));
    return vit_validate(d, dinov2_form(n_prefix));
}

extern "C" size_t slime_dinov2_workspace_bytes(const slime_vit_desc* d, int n_prefix, int n_crops) {
    return n_prefix >= 1 && n_prefix <= 17 ? vit_workspace(d, n_crops, nullptr, dinov2_form(n_prefix)) : 0;
}

extern "C" size_t slime_dinov2_ksplit_workspace_bytes(const slime_vit_desc* d, int n_prefix, int n_crops, const slime_vit_ksplit* ks) {
    return ks && n_prefix >= 1 && n_prefix <= 17 ? vit_workspace(d, n_crops, ks, dinov2_form(n_prefix)) : 0;
}

extern "C" int slime_dinov2_forward(const slime_vit_desc* d, int n_prefix, const void* pixels, int pix_dtype, int n, void* out, int out_dtype,
                                    int keep_prefix, float* hidden_f32, float* states_f32, const slime_vit_ksplit* ks, void* ws,
                                    size_t ws_bytes, void* stream) {
    TRY(dinov2_prefix_ok(n_prefix));
    return vit_run(d, pixels, pix_dtype, n, out, out_dtype, keep_prefix, hidden_f32, ws, ws_bytes, stream, nullptr, states_f32, ks,
                   dinov2_form(n_prefix));
}

// ------------------------------------------------------------------------------------------------
// Resampler
// ------------------------------------------------------------------------------------------------
static int resampler_validate(const slime_resampler_desc* d) {
    SLIME_REQUIRE(d, "resampler: null descriptor");
    SLIME_REQUIRE(is16(d->dtype), "resampler: dtype must be BF16 or F16");
    SLIME_REQUIRE(d->dim == 128 || d->dim == 256 || d->dim == 1024, "resampler: dim=%d unsupported", d->dim);
    SLIME_REQUIRE(d->heads > 0 && d->dim % d->heads == 0, "resampler: heads");
    const int dh = d->dim / d->heads;
    SLIME_REQUIRE(dh == 64 || dh == 128, "resampler: head_dim %d unsupported", dh);
    SLIME_REQUIRE(d->n_query > 0 && d->n_kv > 0, "resampler: empty query/key grid");
    // a projection weight is given as its row-major image, its fragment-order image, or both (slime_gemm_b_frag_usable)
    SLIME_REQUIRE(d->q_proj && d->pos_k && d->ln_kv_w && d->ln_kv_b && (d->w_k || d->w_k_frag) && d->b_k && (d->w_v || d->w_v_frag) && d->b_v &&
                  (d->w_o || d->w_o_frag) && d->b_o && d->ln_post_w && d->ln_post_b, "resampler: missing weights");
    return SLIME_OK;
}

struct ResPlan { size_t xn, xk, kp, vp, ctx, o32, total; };
static ResPlan res_plan(const slime_resampler_desc* d, int n) {
    const size_t Rk = (size_t)n * d->n_kv, Rq = (size_t)n * d->n_query, D = d->dim;
    ResPlan p{};
    size_t off = 0;
    auto take = [&](size_t b) { size_t o = align_up(off, 256); off = o + b; return o; };
    p.xn = take(Rk * D * 2); p.xk = take(Rk * D * 2); p.kp = take(Rk * D * 2); p.vp = take(Rk * D * 2);
    p.ctx = take(Rq * D * 2); p.o32 = take(Rq * D * 4);
    p.total = align_up(off, 256);
    return p;
}

extern "C" size_t slime_resampler_workspace_bytes(const slime_resampler_desc* d, int n) {
    if (!d || n <= 0) return 0;
    return res_plan(d, n).total;
}

int layernorm_crops_launch(const void* feats, int dtype, int P, int period, int first, int per_image, int images, int D, const float* w,
                           const float* b, float eps, void* out_t, void* out_t2, const float* add, int add_period, void* stream);   // rowwise.hip (internal)

// A crop source of the fused adapter: crop j of the n selected crops is crop (j / per_image) * period + first + j % per_image of the
// tower's T features (a uniform batch), or crop table[j] (table != nullptr, a DEVICE int32 array: the ragged batch)
struct ResCrops { const void* feats; int period, first, per_image, images; const int* table = nullptr; };
// crops != nullptr (fused adapter, round 5): the input rows are those crops, read by the first LayerNorm directly (no fp32 copy of
// them); otherwise x fp32 [n, n_kv, dim]
static int resampler_run(const slime_resampler_desc* d, const float* x, int ldx, const ResCrops* crops, int n, float* out_f32,
                         void* out_t, void* ws, size_t ws_bytes, void* stream) {
    TRY(resampler_validate(d));
    SLIME_REQUIRE((x || crops) && n > 0 && (crops || ldx >= d->dim), "resampler: bad input");
    SLIME_REQUIRE(out_f32 || out_t, "resampler: no output requested");
    const ResPlan p = res_plan(d, n);
    TRY(ws_check("resampler", ws, ws_bytes, p.total));
    char* w = (char*)ws;
    const int D = d->dim, Rk = n * d->n_kv, Rq = n * d->n_query, dh = D / d->heads, dt = d->dtype;
    // x = ln_kv(x); K input = x + pos (sampler.py:158,164); V input = x
    if (crops && crops->table)
        TRY(layernorm_crops_indexed_launch(crops->feats, dt, d->n_kv, crops->table, n, D, d->ln_kv_w, d->ln_kv_b, d->eps, w + p.xn, w + p.xk,
                                           d->pos_k, d->n_kv, stream));
    else if (crops)
        TRY(layernorm_crops_launch(crops->feats, dt, d->n_kv, crops->period, crops->first, crops->per_image, crops->images, D, d->ln_kv_w,
                                   d->ln_kv_b, d->eps, w + p.xn, w + p.xk, d->pos_k, d->n_kv, stream));
    else
        TRY(slime_layernorm(x, ldx, Rk, D, d->ln_kv_w, d->ln_kv_b, d->eps, 1, nullptr, w + p.xn, w + p.xk, d->pos_k,
                            d->n_kv, dt, stream));
    TRY(gemm_w(w + p.xk, D, d->w_k, d->w_k_frag, d->b_k, w + p.kp, D, Rk, D, D, dt, SLIME_EPI_BIAS_T, stream));
    TRY(gemm_w(w + p.xn, D, d->w_v, d->w_v_frag, d->b_v, w + p.vp, D, Rk, D, D, dt, SLIME_EPI_BIAS_T, stream));
    TRY(slime_attention(d->q_proj, 0, D, w + p.kp, (long)d->n_kv * D, D, w + p.vp, (long)d->n_kv * D, D, w + p.ctx,
                        (long)d->n_query * D, D, n, d->heads, dh, d->n_query, d->n_kv, dt, stream));
    TRY(gemm_w(w + p.ctx, D, d->w_o, d->w_o_frag, d->b_o, w + p.o32, D, Rq, D, D, dt, SLIME_EPI_BIAS_F32, stream));
    TRY(slime_layernorm((const float*)(w + p.o32), D, Rq, D, d->ln_post_w, d->ln_post_b, d->eps, 1, out_f32, out_t,
                        nullptr, nullptr, 0, dt, stream));
    return SLIME_OK;
}

extern "C" int slime_resampler_forward(const slime_resampler_desc* d, const float* x, int ldx, int n, float* out_f32,
                                       void* out_t, void* ws, size_t ws_bytes, void* stream) {
    SLIME_REQUIRE(x, "resampler: bad input");
    return resampler_run(d, x, ldx, nullptr, n, out_f32, out_t, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// Projector MLP
// ------------------------------------------------------------------------------------------------
static int mlp_validate(const slime_mlp_desc* d) {
    SLIME_REQUIRE(d, "mlp: null descriptor");
    SLIME_REQUIRE(is16(d->dtype), "mlp: dtype must be BF16 or F16");
    SLIME_REQUIRE(d->in_dim == 128 || d->in_dim == 256 || d->in_dim == 768 || d->in_dim == 1024, "mlp: in_dim=%d unsupported", d->in_dim);
    SLIME_REQUIRE(d->hidden % 128 == 0, "mlp: hidden=%d must be a multiple of 128", d->hidden);
    SLIME_REQUIRE((d->w1 || d->w1_frag) && d->b1 && (d->w2 || d->w2_frag) && d->b2, "mlp: missing weights (row-major or fragment-order)");
    return SLIME_OK;
}

struct MlpPlan { size_t xt, mid, total; };
static MlpPlan mlp_plan(const slime_mlp_desc* d, int rows) {
    MlpPlan p{};
    size_t off = 0;
    auto take = [&](size_t b) { size_t o = align_up(off, 256); off = o + b; return o; };
    p.xt = take((size_t)rows * d->in_dim * 2);
    p.mid = take((size_t)rows * d->hidden * 2);
    p.total = align_up(off, 256);
    return p;
}

extern "C" size_t slime_mlp_workspace_bytes(const slime_mlp_desc* d, int rows) {
    if (!d || rows <= 0) return 0;
    return mlp_plan(d, rows).total;
}

extern "C" int slime_mlp_forward(const slime_mlp_desc* d, const float* x_f32, const void* x_t, int rows, float* out,
                                 void* ws, size_t ws_bytes, void* stream) {
    TRY(mlp_validate(d));
    SLIME_REQUIRE((x_f32 || x_t) && out && rows > 0, "mlp: bad input");
    const MlpPlan p = mlp_plan(d, rows);
    TRY(ws_check("mlp", ws, ws_bytes, p.total));
    char* w = (char*)ws;
    const void* a = x_t;
    if (!a) {
        TRY(slime_layernorm(x_f32, d->in_dim, rows, d->in_dim, nullptr, nullptr, 0.f, 0, nullptr, w + p.xt, nullptr,
                            nullptr, 0, d->dtype, stream));
        a = w + p.xt;
    }
    TRY(gemm_w(a, d->in_dim, d->w1, d->w1_frag, d->b1, w + p.mid, d->hidden, rows, d->hidden, d->in_dim, d->dtype,
                   SLIME_EPI_BIAS_GELU_T, stream));
    TRY(gemm_w(w + p.mid, d->hidden, d->w2, d->w2_frag, d->b2, out, d->hidden, rows, d->hidden, d->hidden, d->dtype,
                   SLIME_EPI_BIAS_F32, stream));
    return SLIME_OK;
}

// ------------------------------------------------------------------------------------------------
// GatedBlock
// ------------------------------------------------------------------------------------------------
struct GatedPlan { size_t stack, mlp, res, gates, total; };
static GatedPlan gated_plan(const slime_mlp_desc* m, const slime_resampler_desc* r, int n) {
    const size_t rows = (size_t)n * r->n_query;
    GatedPlan p{};
    size_t off = 0;
    auto take = [&](size_t b) { size_t o = align_up(off, 256); off = o + b; return o; };
    p.stack = take(2 * rows * m->in_dim * 2);                  // [T(x) | attn(x)]: the MLP's stacked operand
    p.mlp = take(mlp_plan(m, (int)(2 * rows)).total);
    p.res = take(res_plan(r, n).total);
    p.gates = take(rows * 2 * sizeof(float));
    p.total = align_up(off, 256);
    return p;
}

extern "C" size_t slime_gated_workspace_bytes(const slime_mlp_desc* mlp, const slime_resampler_desc* attn, int n) {
    if (!mlp || !attn || n <= 0) return 0;
    return gated_plan(mlp, attn, n).total;
}

// Both experts, mixed by the gate (builder.py:190-206).  projection[0] + GELU run over the stacked rows [T(x) | attn(x) | local rows]
// (row offsets seg_x = 0, seg_attn, seg_local; seg_local < 0: no local rows); the gate, from the fp32 global rows x32, mixes the
// HIDDEN rows of the two global segments into the second one (slime_gate_premix: projection[2] is linear and g0 + g1 =
// 1 / (1 + 1e-6)), so projection[2] runs over ONE row per token -- a third less GEMM work than two complete experts (round 4).
// Returns projection[2]'s A operand, the [mixed global | local] rows of `mid`, and its row count.
static int both_experts_hidden(const slime_mlp_desc* mlp, const float* w_gate, const char* stack, long seg_x, long seg_attn, long seg_local,
                               long rows_g, long rows_l, const float* x32, float* gates, char* mid, void* stream, const void** a2, int* rows2) {
    const int D = mlp->in_dim, H = mlp->hidden, dt = mlp->dtype;
    char* mixed = mid + (size_t)seg_attn * H * 2;
    if (mix_in_gemm(mlp)) {
        // the mix in fp32 inside projection[0]'s epilogue (SLIME_EPI_BIAS_GELU_MIX_T: one rounding, no pass over the hidden rows,
        // half the global hidden rows written); the local rows follow in their own launch, directly behind the mixed rows
        TRY(slime_gate_weights(x32, D, w_gate, gates, (int)rows_g, stream));
        TRY(gemm_mix(stack + (size_t)seg_x * D * 2, stack + (size_t)seg_attn * D * 2, gates, mlp, mixed, (int)rows_g, stream));
        if (seg_local >= 0)
            TRY(gemm_w(stack + (size_t)seg_local * D * 2, D, mlp->w1, mlp->w1_frag, mlp->b1, mid + (size_t)seg_local * H * 2, H,
                       (int)rows_l, H, D, dt, SLIME_EPI_BIAS_GELU_T, stream));
    } else {
        TRY(gemm_w(stack, D, mlp->w1, mlp->w1_frag, mlp->b1, mid, H, (int)(2 * rows_g + rows_l), H, D, dt, SLIME_EPI_BIAS_GELU_T, stream));
        TRY(slime_gate_premix(x32, D, w_gate, mid + (size_t)seg_x * H * 2, mixed, mixed, dt, (int)rows_g, H, stream));
    }
    *a2 = mixed;
    *rows2 = (int)(rows_g + rows_l);
    return SLIME_OK;
}

extern "C" int slime_gated_forward(const slime_mlp_desc* mlp, const slime_resampler_desc* attn, const float* w_gate,
                                   int learnable_gated, const float* x, int n, float* out, void* ws, size_t ws_bytes,
                                   void* stream) {
    TRY(mlp_validate(mlp));
    TRY(resampler_validate(attn));
    SLIME_REQUIRE(x && out && n > 0, "gated: bad input");
    SLIME_REQUIRE(attn->dim == mlp->in_dim && attn->n_query == attn->n_kv, "gated: attn must map the token grid onto itself");
    SLIME_REQUIRE(learnable_gated >= 0 || w_gate, "gated: missing w_gate");
    SLIME_REQUIRE(learnable_gated <= 1, "gated: expert index %d", learnable_gated);
    const GatedPlan p = gated_plan(mlp, attn, n);
    TRY(ws_check("gated", ws, ws_bytes, p.total));
    char* w = (char*)ws;
    const int rows = n * attn->n_query, D = mlp->in_dim, H = mlp->hidden, dt = mlp->dtype;
    const MlpPlan mp = mlp_plan(mlp, 2 * rows);
    const size_t res_ws = res_plan(attn, n).total;
    char* stack = w + p.stack;
    char* attn_t = stack + (size_t)rows * D * 2;
    if (learnable_gated == 0)                                   // expert 0: projection(x)
        return slime_mlp_forward(mlp, x, nullptr, rows, out, w + p.mlp, mp.total, stream);
    TRY(slime_resampler_forward(attn, x, attn->dim, n, nullptr, attn_t, w + p.res, res_ws, stream));
    if (learnable_gated == 1)                                   // expert 1: projection(attn(x))
        return slime_mlp_forward(mlp, nullptr, attn_t, rows, out, w + p.mlp, mp.total, stream);
    // both experts: the block's output is projection[2] over the mixed hidden rows
    const void* a2;
    int rows2;
    TRY(slime_layernorm(x, D, rows, D, nullptr, nullptr, 0.f, 0, nullptr, stack, nullptr, nullptr, 0, dt, stream));
    TRY(both_experts_hidden(mlp, w_gate, stack, 0, rows, -1, rows, 0, x, (float*)(w + p.gates), w + p.mlp + mp.mid, stream, &a2, &rows2));
    TRY(gemm_w(a2, H, mlp->w2, mlp->w2_frag, mlp->b2, out, H, rows2, H, H, dt, SLIME_EPI_BIAS_F32, stream));
    return SLIME_OK;
}

// ------------------------------------------------------------------------------------------------
// Fused adapter (GatedBlock on the global crops + post_qformer/MLP/merge on the local crops)
// ------------------------------------------------------------------------------------------------
int adapter_row_map_launch(int* map, long rows_g, int P, long rows_l, long per_image_local, int g, int nw, int merge, long out_image_stride,
                           void* stream);                                   // rowwise.hip (internal)
struct AdapterPlan {
    size_t xg32, stack, e, mlp, res, gates, rmap, total;    // offsets
    long rows_g, rows_l, rows_all, total_local;
    int n_images, segs_g;
    long seg_x, seg_attn, seg_local;                        // first row of each segment of the stack (-1: dropped)
};
// total_local = local crops of the whole batch (n_images * n_local for a uniform batch, sum n_i for a ragged one)
static AdapterPlan adapter_plan_total(const slime_mlp_desc* m, const slime_resampler_desc* attn, const slime_resampler_desc* post,
                                      int n_images, long total_local, int learnable_gated) {
    AdapterPlan p{};
    const size_t D = m->in_dim, H = m->hidden;
    p.n_images = n_images;
    p.total_local = total_local;
    p.rows_g = (long)n_images * attn->n_kv;
    p.rows_l = post ? total_local * post->n_query : 0;
    p.segs_g = learnable_gated < 0 ? 2 : 1;
    p.rows_all = p.segs_g * p.rows_g + p.rows_l;
    // stacked MLP input: [x_global | attn(x_global) | post_qformer(x_local)] (segments that are not needed are dropped)
    p.seg_x = learnable_gated != 1 ? 0 : -1;
    p.seg_attn = learnable_gated != 0 ? (p.segs_g - 1) * p.rows_g : -1;
    p.seg_local = post ? p.segs_g * p.rows_g : -1;
    size_t off = 0;
    auto take = [&](size_t b) { size_t o = align_up(off, 256); off = o + b; return o; };
    p.xg32 = take((size_t)p.rows_g * D * 4);
    p.stack = take((size_t)p.rows_all * D * 2);
    p.e = take((size_t)p.rows_all * H * 4);
    p.mlp = take(mlp_plan(m, (int)p.rows_all).total);
    size_t res = res_plan(attn, n_images).total;
    if (post && total_local > 0) { const size_t r2 = res_plan(post, (int)total_local).total; if (r2 > res) res = r2; }
    p.res = take(res);
    p.gates = take((size_t)p.rows_g * 2 * sizeof(float));
    p.rmap = take((size_t)(p.rows_g + p.rows_l) * sizeof(int));
    p.total = align_up(off, 256);
    return p;
}
static AdapterPlan adapter_plan(const slime_mlp_desc* m, const slime_resampler_desc* attn, const slime_resampler_desc* post,
                                int n_images, int n_local, int learnable_gated) {
    return adapter_plan_total(m, attn, post, n_images, (long)n_images * n_local, learnable_gated);
}

extern "C" size_t slime_adapter_workspace_bytes(const slime_mlp_desc* mlp, const slime_resampler_desc* attn,
                                                const slime_resampler_desc* post, int n_images, int n_local) {
    if (!mlp || !attn || n_images <= 0 || n_local < 0 || (n_local > 0 && !post)) return 0;
    return adapter_plan(mlp, attn, n_local > 0 ? post : nullptr, n_images, n_local, -1).total;
}

// The checks the uniform and the ragged entry share (`who`: the entry's own prefix, for its bad-input message)
static int adapter_validate(const slime_mlp_desc* mlp, const slime_resampler_desc* attn, const float* w_gate, int learnable_gated,
                            bool args_ok, const char* who) {
    TRY(mlp_validate(mlp));
    TRY(resampler_validate(attn));
    SLIME_REQUIRE(args_ok, "%s: bad input", who);
    SLIME_REQUIRE(attn->dim == mlp->in_dim && attn->n_query == attn->n_kv, "adapter: attn must map the token grid onto itself");
    SLIME_REQUIRE(learnable_gated >= 0 || w_gate, "adapter: missing w_gate");
    SLIME_REQUIRE(learnable_gated <= 1, "adapter: expert index %d", learnable_gated);
    SLIME_REQUIRE(attn->dtype == mlp->dtype, "adapter: mixed operand dtypes");
    return SLIME_OK;
}
// ... and, where the batch has local crops, post_qformer against the tower grid; *g = the side of its square query grid
static int adapter_validate_post(const slime_mlp_desc* mlp, const slime_resampler_desc* attn, const slime_resampler_desc* post, int* g) {
    TRY(resampler_validate(post));
    SLIME_REQUIRE(post->dim == mlp->in_dim && post->n_kv == attn->n_kv && post->dtype == mlp->dtype, "adapter: post_qformer does not match the tower grid");
    int s = 0;
    while (s * s < post->n_query) ++s;
    SLIME_REQUIRE(s * s == post->n_query, "adapter: post_qformer query count %d is not a square grid", post->n_query);
    *g = s;
    return SLIME_OK;
}

// The adapter's launch sequence, the one body behind slime_adapter_forward and slime_adapter_forward_ragged: global crop select ->
// attn resampler -> post_qformer on the local crops -> projection[0] over the stack (with the gate mix where both experts run) ->
// projection[2].  `glob` / `local` say where a crop's features come from (window arithmetic or a device table).  projection[2]
// stores every row straight into the token buffer `out` through `row_map` (round 5; slime_gemm_args.row_map: global rows to rows
// [0, P) of their image, local rows to their raster position behind them), rounded once by the same RNE pack as the merge kernel's:
// bit-identical to the per-module sequence.  row_map == nullptr: plain [global | local] rows to `out`, for the caller to merge.
// `uniform` != nullptr: row_map is still to be built, by adapter_row_map_launch from these numbers, where the uniform call has always
// launched it -- behind the resamplers (a ragged batch's plan kernel, which also writes the crop tables, has to run before the body).
struct UniformRows { long per_image_local, out_image_stride; int g, nw, merge; };
static int adapter_run(const slime_mlp_desc* mlp, const slime_resampler_desc* attn, const float* w_gate, const slime_resampler_desc* post,
                       const AdapterPlan& p, char* w, const ResCrops& glob, const ResCrops& local, const UniformRows* uniform, int* row_map,
                       void* out, int out_dtype, void* stream) {
    const int P = attn->n_kv, D = mlp->in_dim, H = mlp->hidden, dt = mlp->dtype;
    float* xg32 = (float*)(w + p.xg32);
    char* stack = w + p.stack;
    auto seg = [&](long s) { return stack + (size_t)s * D * 2; };
    // global crops: fp32 copy for the resampler's LayerNorm and the gate logits, T copy straight into the stack
    void* x_t = p.seg_x >= 0 ? seg(p.seg_x) : nullptr;
    if (glob.table)
        TRY(select_crops_indexed_launch(glob.feats, dt, P, D, glob.table, p.n_images, xg32, x_t, stream));
    else
        TRY(slime_select_crops(glob.feats, dt, P, D, glob.period, glob.first, glob.per_image, glob.images, xg32, x_t, stream));
    if (p.seg_attn >= 0)
        TRY(slime_resampler_forward(attn, xg32, D, p.n_images, nullptr, seg(p.seg_attn), w + p.res, res_plan(attn, p.n_images).total, stream));
    if (post)
        // local crops: post_qformer's first LayerNorm reads them straight from the tower's T features (round 5: no fp32 copy --
        // 75 MB written and read back per 8 x (1+4) step --, no select_crops launch; float(T) either way: bit-identical)
        TRY(resampler_run(post, nullptr, 0, &local, (int)p.total_local, nullptr, seg(p.seg_local), w + p.res,
                          res_plan(post, (int)p.total_local).total, stream));
    if (uniform)
        TRY(adapter_row_map_launch(row_map, p.rows_g, P, p.rows_l, uniform->per_image_local, uniform->g, uniform->nw, uniform->merge,
                                   uniform->out_image_stride, stream));
    // projection MLP over the stack: projection[2] runs over one row per output token, [mixed global | local] with both experts
    char* mid = w + p.mlp + mlp_plan(mlp, (int)p.rows_all).mid;
    const void* a2 = mid;
    int rows2 = (int)p.rows_all;
    if (p.segs_g == 2)
        TRY(both_experts_hidden(mlp, w_gate, stack, p.seg_x, p.seg_attn, p.seg_local, p.rows_g, p.rows_l, xg32, (float*)(w + p.gates), mid,
                                stream, &a2, &rows2));
    else
        TRY(gemm_w(stack, D, mlp->w1, mlp->w1_frag, mlp->b1, mid, H, rows2, H, D, dt, SLIME_EPI_BIAS_GELU_T, stream));
    slime_gemm_args a{};
    a.A = a2; a.lda = H; a.B = mlp->w2; a.B_frag = mlp->w2_frag; a.bias = mlp->b2; a.M = rows2; a.N = H; a.K = H; a.dtype = dt;
    a.C = out; a.ldc = H; a.row_map = row_map; a.epilogue = out_dtype == SLIME_F32 ? SLIME_EPI_BIAS_F32 : SLIME_EPI_BIAS_T;
    return slime_gemm_ex(&a, stream);
}

// A batch whose images share one crop layout (1 global + n_local = nw x nh local crops each)
extern "C" int slime_adapter_forward(const slime_mlp_desc* mlp, const slime_resampler_desc* attn, const float* w_gate,
                                     int learnable_gated, const slime_resampler_desc* post, const void* feats,
                                     int n_images, int n_local, int nw, int nh, int merge, void* out, int out_dtype,
                                     long out_image_stride, void* ws, size_t ws_bytes, void* stream) {
    TRY(adapter_validate(mlp, attn, w_gate, learnable_gated, feats && out && n_images > 0 && n_local >= 0, "adapter"));
    int g = 1;
    if (n_local > 0) {
        TRY(adapter_validate_post(mlp, attn, post, &g));
        SLIME_REQUIRE(nw > 0 && nh > 0 && nw * nh == n_local, "adapter: grid %dx%d does not hold %d local crops", nw, nh, n_local);
    } else {
        post = nullptr;
    }
    const int P = attn->n_kv, H = mlp->hidden;
    const long per_image_local = post ? (long)n_local * post->n_query : 0;
    const AdapterPlan p = adapter_plan(mlp, attn, post, n_images, n_local, learnable_gated);
    SLIME_REQUIRE(out_image_stride >= P + per_image_local, "adapter: out_image_stride %ld too small", out_image_stride);
    // (the direct store's limit; checked here, with every other argument, before the first launch)
    const bool direct = out_dtype == SLIME_F32 || out_dtype == mlp->dtype;
    SLIME_REQUIRE(!direct || (long)n_images * out_image_stride < (1L << 31), "adapter: token buffer too large for the 32-bit row map");
    TRY(ws_check("adapter", ws, ws_bytes, p.total));
    char* w = (char*)ws;
    const ResCrops glob{feats, 1 + n_local, 0, 1, n_images}, local{feats, 1 + n_local, 1, n_local, n_images};
    if (direct) {
        const UniformRows rows{post ? per_image_local : 1, out_image_stride, g, nw > 0 ? nw : 1, merge};
        return adapter_run(mlp, attn, w_gate, post, p, w, glob, local, &rows, (int*)(w + p.rmap), out, out_dtype, stream);
    }
    // A 16-bit output type that is not the operand type keeps the fp32 rows e = [global | local] and the merge passes.
    float* e = (float*)(w + p.e);
    TRY(adapter_run(mlp, attn, w_gate, post, p, w, glob, local, nullptr, nullptr, e, SLIME_F32, stream));
    // global tokens -> rows [0, P) of every image: flat cast-copy of P rows per image (nw = P, nh = g = 1, merge = 0)
    TRY(slime_merge_rows_batched(e, P, out, out_dtype, out_image_stride, 0, n_images, P, 1, 1, H, 0, stream));
    if (post)
        TRY(slime_merge_rows_batched(e + (size_t)p.rows_g * H, per_image_local, out, out_dtype, out_image_stride, P, n_images, nw, nh, g, H,
                                     merge, stream));
    return SLIME_OK;
}

// ------------------------------------------------------------------------------------------------
// Fused adapter for a batch whose images have DIFFERENT crop layouts: a second front end of adapter_run.  The three places that
// assume one layout -- the crops' positions in feats, the rows each image owns in the token buffer, its crop grid -- are read from
// device tables that ONE plan kernel derives from the per-image layout in its kernel arguments: the two crop tables are adapter_run's
// crop sources, the third its row map.  Every launch after the plan kernel is the shared body's; the rows are independent, so an
// image's tokens are those of the uniform call on that image alone up to the GEMM's tile choice.
// ------------------------------------------------------------------------------------------------
struct RaggedPlan { AdapterPlan a; size_t gtab, ltab, total; };

// host-only: validates the grids and fills the layout (out_row0 == nullptr: packed); *post is cleared when no image has local crops
static int ragged_layout(const slime_mlp_desc* mlp, const slime_resampler_desc* attn, const slime_resampler_desc** post, int n_images,
                         const int* nw, const int* nh, int merge, const long long* out_row0, long out_rows, RaggedLayout* L) {
    SLIME_REQUIRE(n_images > 0 && nw && nh, "adapter_ragged: bad input");
    SLIME_REQUIRE(n_images <= SLIME_ADAPTER_RAGGED_MAX_IMAGES, "adapter_ragged: %d images, more than SLIME_ADAPTER_RAGGED_MAX_IMAGES = %d (the layout "
                  "travels in the kernel arguments)", n_images, SLIME_ADAPTER_RAGGED_MAX_IMAGES);
    long total_local = 0;
    for (int i = 0; i < n_images; ++i) {
        SLIME_REQUIRE(nw[i] >= 0 && nh[i] >= 0 && (nw[i] == 0) == (nh[i] == 0), "adapter_ragged: image %d: grid %dx%d (a grid is 0x0 -- no local "
                      "crops -- or has both factors > 0)", i, nw[i], nh[i]);
        SLIME_REQUIRE((long)nw[i] * nh[i] <= (1 << 16), "adapter_ragged: image %d: grid %dx%d holds more than 65536 crops", i, nw[i], nh[i]);
        total_local += (long)nw[i] * nh[i];
    }
    int g = 1, q = 1;
    if (total_local > 0) {
        SLIME_REQUIRE(*post, "adapter_ragged: local crops without post_qformer");
        TRY(adapter_validate_post(mlp, attn, *post, &g));
        q = (*post)->n_query;
    } else {
        *post = nullptr;
    }
    const int P = attn->n_kv;
    SLIME_REQUIRE(out_rows > 0 && out_rows < (1L << 31), "adapter_ragged: token buffer of %ld rows is beyond the 32-bit row map (limit 2^31 - 1 rows)", out_rows);
    SLIME_REQUIRE(((long)n_images * P + total_local * q) < (1L << 31), "adapter_ragged: %ld token rows are beyond the 32-bit row map", (long)n_images * P + total_local * q);
    *L = RaggedLayout{};
    L->n_images = n_images; L->P = P; L->q = q; L->g = g; L->merge = merge ? 1 : 0;
    long crop = 0, lrow = 0, packed = 0;
    for (int i = 0; i < n_images; ++i) {
        const long n = (long)nw[i] * nh[i], rows = P + n * q;
        const long long r0 = out_row0 ? out_row0[i] : (long long)packed;
        SLIME_REQUIRE(rows <= out_rows && r0 >= 0 && r0 <= out_rows - rows, "adapter_ragged: image %d: %ld rows from row %lld are outside the token "
                      "buffer (out_rows = %ld%s)", i, rows, r0, out_rows, out_row0 ? "" : ": too small for the packed images");
        L->crop0[i] = (int)crop; L->n[i] = (int)n; L->nw[i] = nw[i] > 0 ? nw[i] : 1; L->dst0[i] = (int)r0; L->lrow0[i] = (int)lrow;
        crop += 1 + n; lrow += n * q; packed += rows;
    }
    L->lrow0[n_images] = (int)lrow;
    if (out_row0)                                                // explicit rows: no two images may share a row (64 images: the plain pair test)
        for (int i = 0; i < n_images; ++i)
            for (int j = 0; j < i; ++j) {
                const long ri = L->dst0[i], ei = ri + P + (long)L->n[i] * q, rj = L->dst0[j], ej = rj + P + (long)L->n[j] * q;
                SLIME_REQUIRE(ei <= rj || ej <= ri, "adapter_ragged: out_row0 of images %d and %d overlap (rows [%ld, %ld) and [%ld, %ld))", j, i, rj, ej, ri, ei);
            }
    return SLIME_OK;
}

static RaggedPlan ragged_plan(const slime_mlp_desc* m, const slime_resampler_desc* attn, const slime_resampler_desc* post, int n_images,
                              long total_local, int learnable_gated) {
    RaggedPlan p{};
    p.a = adapter_plan_total(m, attn, post, n_images, total_local, learnable_gated);
    p.gtab = p.a.total;                                          // 256-B aligned
    p.ltab = p.gtab + align_up((size_t)n_images * sizeof(int), 256);
    p.total = p.ltab + align_up((size_t)total_local * sizeof(int), 256);
    return p;
}

extern "C" size_t slime_adapter_ragged_workspace_bytes(const slime_mlp_desc* mlp, const slime_resampler_desc* attn,
                                                       const slime_resampler_desc* post, int n_images, const int* nw, const int* nh) {
    if (!mlp || !attn || !nw || !nh || n_images <= 0 || n_images > SLIME_ADAPTER_RAGGED_MAX_IMAGES) return 0;
    long total_local = 0;
    for (int i = 0; i < n_images; ++i) {
        if (nw[i] < 0 || nh[i] < 0 || (nw[i] == 0) != (nh[i] == 0) || (long)nw[i] * nh[i] > (1 << 16)) return 0;
        total_local += (long)nw[i] * nh[i];
    }
    if (total_local > 0 && !post) return 0;
    return ragged_plan(mlp, attn, total_local > 0 ? post : nullptr, n_images, total_local, -1).total;
}

extern "C" int slime_adapter_forward_ragged(const slime_mlp_desc* mlp, const slime_resampler_desc* attn, const float* w_gate,
                                            int learnable_gated, const slime_resampler_desc* post, const void* feats, int n_images,
                                            const int* nw, const int* nh, int merge, void* out, int out_dtype,
                                            const long long* out_row0, long out_rows, void* ws, size_t ws_bytes, void* stream) {
    TRY(adapter_validate(mlp, attn, w_gate, learnable_gated, feats && out, "adapter_ragged"));
    SLIME_REQUIRE(out_dtype == SLIME_F32 || out_dtype == mlp->dtype, "adapter_ragged: out_dtype %d is neither fp32 nor the operand type %d (a 16-bit "
                  "output type other than the operand type is not stored through the row map: use the per-module path)", out_dtype, mlp->dtype);
    RaggedLayout L;
    TRY(ragged_layout(mlp, attn, &post, n_images, nw, nh, merge, out_row0, out_rows, &L));
    const RaggedPlan rp = ragged_plan(mlp, attn, post, n_images, L.lrow0[n_images] / L.q, learnable_gated);
    TRY(ws_check("adapter_ragged", ws, ws_bytes, rp.total));
    char* w = (char*)ws;
    int* rmap = (int*)(w + rp.a.rmap);
    int* gtab = (int*)(w + rp.gtab);
    int* ltab = (int*)(w + rp.ltab);
    // the device tables: projection[2]'s row map and the source crops of the global / local segments
    TRY(adapter_ragged_plan_launch(L, rmap, gtab, ltab, stream));
    const ResCrops glob{feats, 0, 0, 0, 0, gtab}, local{feats, 0, 0, 0, 0, ltab};
    return adapter_run(mlp, attn, w_gate, post, rp.a, w, glob, local, nullptr, rmap, out, out_dtype, stream);
}
