// Host-side executors of the two frozen encoders: enqueue the kernel chain of one ViT / BERT forward on the
// caller's stream and write the per-layer CLS taps in one pass (no hidden state other than the live one is kept).
// Replaces Vit_Encoder.forward / Bert_Encoder.forward + `hidden_states[i][:,0]`
// (Code_Uncached/model/encoders.py:29-31,81-91,148-159; model.py:210-213) — and, run over a catalogue, what
// Code_Cached/preprocess_vectors.py:68-112 precomputes.
#include "common.h"

namespace {

struct EncBufs {
    float* X;       // [Tp, D] fp32 residual stream (resid32 mode; in the default mixed mode: the patch embedding's output only,
                    // aliased onto QKV, which is first written after block 0's LN1 has consumed it)
    void* X16;      // [Tp, D] fp16: residual stream of the non-CLS rows (mixed mode)
    float* Xc;      // [Mcp, D] fp32: residual stream of the CLS rows, compact (mixed mode) = the hidden states' tapped rows
    void* H;        // [Tp, D] 16-bit: LayerNorm output, reused as the attention context
    void* QKV;      // [Tp, 3D] 16-bit: head-major per item (EPI_QKVH16); 80-wide heads: row-major, the output of a plain product
    void* F1;       // [Tp, max(F, patch_dim)] 16-bit: GELU(FC1) (and the patch matrix during embedding)
    void* D16;      // [Tp, D] 16-bit: output of the O GEMM (a residual DELTA, added to the fp32 stream by LayerNorm kernels)
    void* D16b;     // [Tp, D] 16-bit: output of the FC2 GEMM
    float* KB;      // [Mc, W] key bias (BERT)
    void* Cls;      // [2, Mcp, D] 16-bit: CLS rows of LN(x) and their Q projection in the CLS-only last block
    int64_t Mcp;    // items per chunk rounded up to a GEMM row tile
    // LayerNorm applied by the consuming product (ViT, fp16, mixed stream; g_ln_fold):
    void* Wf;       // [layers][3D + F, D] fp16: gamma-folded, centred QKV and FC1 weights
    float* Bf;      // [layers][3D + F]: folded biases
    float* RS;      // [Tp]: rstd of every row of the stream
    float* RP;      // [D / 64][Tp][2]: per-slice row sums of the products that add into the stream (EPI_STREAM16)
};

// 1 = keep the whole residual stream in fp32 (rounds 1-3); 0 (default) = fp32 for the CLS rows, fp16 for the others (rowops.hip).
// Bench / test knob (tools/enc_time.py A/B, tests/test_gpu_encoders.py); the *_ws_bytes queries follow it.
int g_resid32 = 0;
// 1 (default): the pre-LN tower (ViT) with fp16 operands and the mixed stream never materialises LayerNorm(x): the add kernels write
// the stream and rstd per row, the QKV / FC1 products read the stream itself against gamma-folded, centred weights and apply
// rstd in their epilogues (Gemm16Args::rowstat) — 12 instead of 16 bytes per token row and block in the HBM-bound kernels.
// 2 (default): ... and no add kernel either: the O / FC2 products add into the fp16 stream in their epilogues (EPI_STREAM16) and leave
// per-slice row sums, a small kernel turns those into rstd and folds the CLS rows' deltas into their fp32 stream.
// 0: the LayerNorm image of rounds 1-4.  Bench / test knob.
int g_ln_fold = 2;
// Block-major ("blk32") intermediates of the persistent 256x256 GEMM.  1: F1, the FC1 -> FC2 intermediate of every
// all-token block of both towers, is written by the FC1 epilogue in accumulator order — every store instruction one whole KiB instead of
// 32 cache lines — and copied as it is into the LDS tile of the FC2 product.  2 (default): ... and the ViT residual stream X16 of the
// product route (VS_STREAM) as well: patches_to_stream writes it block-major, the O / FC2 stream epilogues read-modify-write it, the
// QKV / FC1 products (and the K/V product of the CLS-only last block) stage it, stream_stats_finalize addresses the CLS rows through the
// formula.  0: row-major everywhere (the A/B handle and the tests' reference route: the same kernels, the same arithmetic, bit-equal
// results).
int g_blk32 = 2;
// process-wide OVERRIDE of the weights structs' `full_blocks` field (bench.py, tests; not declared in include/iisan_hip.h):
// 1 = run every block of the tower on every token, as the reference does
int g_full_blocks = 0;

// A call runs in chunks of Mc items; its last chunk may be shorter.  Mc and `last` are the only two chunk sizes a call has.
struct Chunks {
    int64_t Mc, last;
    Chunks(int64_t M, int64_t chunk_items) : Mc((chunk_items > 0 && chunk_items < M) ? chunk_items : M), last(Mc > 0 && M % Mc ? M % Mc : Mc) {}
};

size_t carve(WsCarver& c, EncBufs& b, int64_t tokens, int64_t items, int D, int F, int64_t kb_elems, int fold_layers = 0, bool fold_ws = true) {
    const int64_t Tp = ceil_div(tokens, 256) * 256;     // GEMM A operands are read in 256-row tiles
    b.Mcp = ceil_div(items, 256) * 256;
    b.Cls = c.take<uint16_t>((size_t)2 * b.Mcp * D);
    b.Xc = c.take<float>((size_t)b.Mcp * D);
    b.X16 = c.take<uint16_t>((size_t)Tp * D);
    b.X = g_resid32 ? c.take<float>((size_t)Tp * D) : nullptr;
    b.H = c.take<uint16_t>((size_t)Tp * D);
    b.QKV = c.take<uint16_t>((size_t)Tp * 3 * D);
    if (!b.X) b.X = (float*)b.QKV;                      // 6 bytes per element >= the 4 the fp32 embeddings need
    b.F1 = c.take<uint16_t>((size_t)Tp * F);
    b.D16 = c.take<uint16_t>((size_t)Tp * D);
    b.D16b = c.take<uint16_t>((size_t)Tp * D);
    b.KB = c.take<float>((size_t)(kb_elems > 0 ? kb_elems : 1));
    b.Wf = nullptr; b.Bf = nullptr; b.RS = nullptr; b.RP = nullptr;
    if (fold_layers > 0) {
        if (fold_ws) {          // (not when the caller's weights struct carries the folded set)
            b.Wf = c.take<uint16_t>((size_t)fold_layers * (3 * D + F) * D);
            b.Bf = c.take<float>((size_t)fold_layers * (3 * D + F));
        }
        b.RS = c.take<float>((size_t)Tp);
        b.RP = c.take<float>((size_t)(D / 64) * Tp * 2);
    }
    return c.off;
}

// One 16-bit product: its epilogue mode and its Gemm16Args with everything but the operand pointers.  rowstat / rowpart point at WANTED
// where the product takes them: gemm16_route asks only whether they are there, Chunk::launch puts the workspace buffers in their place.
struct Product { int mode; Gemm16Args a; };
float WANTED;

// The products of one call, each described ONCE: a probe hands a description to gemm16_route, a launch adds the pointers to the same
// description.  The layout decisions of the call are fields, so the probe of a decision is a copy with that decision switched on.
struct Products {
    int dt, D, F, T, heads;
    int act;                // MLP activation of the tower (iisan_vit_weights::act): 0 erf-GELU, 1 quick-GELU — the epilogue mode of every FC1 product
    bool ln = false;        // QKV / FC1 read the stream and apply LayerNorm in their epilogues (VS_FOLD, VS_STREAM)
    bool stream = false;    // O / FC2 add into the stream in their epilogues (VS_STREAM)
    bool f1blk = false;     // F1, the FC1 -> FC2 intermediate of the all-token blocks, is block-major
    bool xblk = false;      // ... and so is the ViT stream X16 (VS_STREAM only)
    // 80-wide heads (ViT-H/14, hidden 1280 = 16 x 80): QKV is a plain row-major product (no GEMM epilogue knows a head width but 64), the
    // attention runs attn16_hd80.hip, and there is no CLS-only form of the last live block: it runs on every token
    bool hd80() const { return D == heads * 80; }
    int fc1_mode() const { return act ? EPI_QGELU16 : EPI_GELU16; }

    // out [M, N] = A [M, K] W^T, natural leading dimensions: the products of the CLS tail (one row per item) as they are
    static Product plain(int mode, int K, int N, int64_t M) {
        Product p{mode, {}};
        p.a.M = M; p.a.N = N; p.a.K = K; p.a.lda = K; p.a.ldw = K; p.a.ldo = N;
        return p;
    }
    // q | k | v from `which0` on, head-major (1: K and V alone, the CLS-only last block)
    Product qkv(int64_t tok, int which0 = 0) const {
        if (hd80()) return plain(EPI_OUT16, D, 3 * D, tok);     // q | k | v only: VitChunk::cls_block, the one caller of which0 = 1, refuses this head width
        Product p = plain(EPI_QKVH16, D, (3 - which0) * D, tok);
        p.a.qkv_S = T; p.a.qkv_heads = heads; p.a.qkv_which0 = which0;
        p.a.rowstat = ln ? &WANTED : nullptr; p.a.a_blk32 = xblk;
        return p;
    }
    Product fc1(int64_t tok) const {
        Product p = plain(fc1_mode(), D, F, tok);
        p.a.rowstat = ln ? &WANTED : nullptr; p.a.a_blk32 = xblk; p.a.out_blk32 = f1blk;
        return p;
    }
    // O (K = D) and FC2 (K = F, A = F1): a 16-bit delta, or x += A W^T + bias in the stream with the row sums of the new rows
    Product to_stream(int K, int64_t tok, bool a_blk) const {
        Product p = plain(stream ? EPI_STREAM16 : EPI_OUT16, K, D, tok);
        p.a.a_blk32 = a_blk;
        if (stream) { p.a.qkv_S = T; p.a.rowpart = &WANTED; p.a.out_blk32 = xblk; }
        return p;
    }
    Product o(int64_t tok) const { return to_stream(D, tok, false); }
    Product fc2(int64_t tok) const { return to_stream(F, tok, f1blk); }
    // patch embedding of `rows` patch vectors of length pd, P per image: fp32 token rows (+ the position table, a pointer) or 16-bit rows
    static Product patch(bool fp32, int pd, int D, int64_t rows, int P) {
        Product p = plain(fp32 ? EPI_PATCH32 : EPI_PATCH16, pd, D, rows);
        p.a.patch_P = P;
        return p;
    }

    // Every product of `list` (P_* bits) on gemm16_h256, for every chunk size of the call?  LayerNorm and the residual add in the epilogue and
    // the block-major operands exist on that kernel alone, and a buffer has ONE layout per call: a product that another kernel would take
    // (gemm16_route: small chunks, forced variants) turns the decision down for the whole call.
    enum { P_QKV = 1, P_KV = 2, P_FC1 = 4, P_O = 8, P_FC2 = 16 };
    bool all_h256(const Chunks& c, int list) const {
        for (int64_t mc : {c.Mc, c.last}) {
            const Product all[] = {qkv(mc * T), qkv(mc * T, 1), fc1(mc * T), o(mc * T), fc2(mc * T)};
            for (int i = 0; i < 5; ++i)
                if ((list >> i & 1) && gemm16_route(dt, all[i].mode, all[i].a) != G16_H256) return false;
        }
        return true;
    }
    // F1 block-major?  Only when both products of the pair take the flag.
    bool f1_blk32(const Chunks& c) const {
        Products t = *this;
        t.f1blk = true;
        return g_blk32 >= 1 && t.all_h256(c, P_FC1 | P_FC2);
    }
};

int tap_index(const int32_t* tap_layers, int n, int layer) {
    for (int k = 0; k < n; ++k)
        if (tap_layers[k] == layer) return k;
    return -1;
}

int max_tap(const int32_t* tap_layers, int n) {
    int m = 0;
    for (int k = 0; k < n; ++k) m = tap_layers[k] > m ? tap_layers[k] : m;
    return m;
}

int check_common(bool vit, int hidden, int layers, int heads, int mlp, int n_taps, const int32_t* tap_layers) {
    // ViT-B / BERT-base, ViT-L / BERT-large, and the narrow towers — BERT-tiny (128), ViT-tiny (192), BERT-mini (256), ViT-small (384);
    // on the ViT executor alone ViT-H/14: 1280 as 16 heads of 80 (1280 as 20 heads of 64 is no tower the reference caches, and stays refused)
    const bool huge = vit && hidden == 1280 && heads == 16;
    IISAN_CHECK_SHAPE(huge || (hidden != 1280 && row_width_instantiated(hidden)),
                      "encoder hidden size %d not supported: the supported widths are 768 (12 heads) and 1024 (16 heads), "
                      "and 128, 192, 256, 384 (2, 3, 4, 6 heads); the ViT executor also takes 1280 as 16 heads of 80", hidden);
    IISAN_CHECK_SHAPE(huge || (heads > 0 && hidden == heads * 64), "encoder head_dim must be 64 (hidden %d, heads %d; supported: 768 / 12 and 1024 / 16, "
                      "128 / 2, 192 / 3, 256 / 4, 384 / 6; ViT only: 1280 / 16, head_dim 80)", hidden, heads);
    IISAN_CHECK_SHAPE(layers >= 1 && layers <= IISAN_MAX_LAYERS, "encoder layers %d out of range", layers);
    IISAN_CHECK_SHAPE(mlp % 128 == 0, "encoder mlp size %d must be a multiple of 128", mlp);
    IISAN_CHECK_SHAPE(n_taps >= 1 && tap_layers, "need at least one tap layer");
    for (int k = 0; k < n_taps; ++k)
        IISAN_CHECK_SHAPE(tap_layers[k] >= 0 && tap_layers[k] <= layers, "tap layer %d outside 0..%d", tap_layers[k], layers);
    return IISAN_OK;
}
// (past 224 tokens the attention steps run the streaming-softmax kernel, attn16_long.hip; everything else takes T as it comes)
int vit_check_tokens(int T) {
    IISAN_CHECK_SHAPE(T <= 1024, "vit: %d tokens per image > 1024 not supported", T);
    return IISAN_OK;
}
int bert_check_words(int words, int max_pos) {
    IISAN_CHECK_SHAPE(words >= 1 && words <= max_pos && words <= 1024, "bert: %d words unsupported (at most max_pos = %d positions, and 1024)", words, max_pos);
    return IISAN_OK;
}

// The LayerNorm-folded routes — fold_ln_weights, the stream statistics, the block-major stream — take fp16 operands and are 768 wide: a
// bf16 tower, a 1024- or 1280-wide one and the narrow ones (128 - 384) run on the LayerNorm-image route whatever ln_fold says, and ask for no folded set.
// So does a CLIP tower at every width: patches_to_stream has no pre-LayerNorm and the <.., LNA> FC1 epilogue no quick-GELU twin
bool vit_fold_routes(int dtype16, int hidden, bool clip) { return dtype16 == IISAN_F16 && hidden == 768 && !clip; }
bool vit_is_clip(const iisan_vit_weights* w) { return w->pre_ln_w != nullptr || w->act != 0; }

// One chunk of a forward: mc items from item m0 of the call on, tok = mc * T token rows, tp = their rows of the tap tensor
struct Chunk : Products {
    const EncBufs& b; hipStream_t s; float eps;
    bool mixed;     // fp32 CLS rows in Xc + a 16-bit stream for the other rows; false: the whole stream fp32 in X (dev knob resid32)
    int64_t m0, mc, tok; float* tp; int n_taps;

    // the description of a product + its pointers
    int launch(Product p, const void* A, const void* W, const float* bias, void* out) const {
        p.a.A = A; p.a.W = W; p.a.bias = bias; p.a.out = out;
        if (p.a.rowstat) p.a.rowstat = b.RS;
        if (p.a.rowpart) p.a.rowpart = b.RP;
        return launch_gemm16(dt, p.mode, p.a, s);
    }
    // the CLS rows of the current hidden state — rows of X at stride T, or the compact CLS stream itself — into tap slot k of n
    int gather_cls(float* out, int n, int k) const {
        return mixed ? launch_gather_cls(b.Xc, out, mc, 1, D, n, k, s) : launch_gather_cls(b.X, out, mc, T, D, n, k, s);
    }
    int tap(int k) const { return gather_cls(tp, n_taps, k); }

    // The last LIVE block when later blocks are dead code, once the tower has put K / V of every token into QKV (head-major; the q third of the
    // buffer is left untouched) and the CLS rows of the block's 16-bit input into Cls: only the CLS token's output is consumed, so Q, attention,
    // O, both adds, FC1 and FC2 run on one row per item; the result, hidden state l + 1 (before any final LayerNorm), goes to
    // tap k.  The towers differ in the attention launch (attn_drop: the train-mode kernel) and in the adds — pre-LN: x += delta, LN2 in front
    // of FC1; post_ln: x = LN(x + keep * delta) with ln1 / ln2.
    // rel != null (DeBERTa): the CLS form of the disentangled attention over the layer's projected tables.
    int cls_tail(const iisan_layer_weights& L, const float* key_bias, const DropCfg* attn_drop, bool post_ln, const RowKeep* keep1,
                 const RowKeep* keep2, int k, const void* rel = nullptr, int span = 0) const {
        void* Qc = (char*)b.Cls + (size_t)b.Mcp * D * 2;       // compact [mc, D] 16-bit views in their own scratch: CLS rows of the input, their Q
        IISAN_TRY(launch(plain(EPI_OUT16, D, D, mc), b.Cls, L.qkv_w, L.qkv_b, Qc));
        if (rel) IISAN_TRY(launch_attention_cls16_disent(dt, b.QKV, rel, key_bias, b.H, mc, T, heads, span, s, Qc));
        else if (attn_drop) IISAN_TRY(launch_attention16_drop(dt, b.QKV, key_bias, b.H, mc, T, heads, *attn_drop, m0, true, Qc, s));
        else IISAN_TRY(launch_attention_cls16(dt, b.QKV, key_bias, b.H, mc, T, heads, s, Qc));
        float* Xc = (float*)b.QKV;      // free once the CLS attention has run (stream order)
        IISAN_TRY(launch(plain(EPI_OUT16, D, D, mc), b.H, L.o_w, L.o_b, b.D16));
        IISAN_TRY(gather_cls(Xc, 1, 0));
        if (post_ln) IISAN_TRY(launch_add_layernorm768(dt, Xc, b.D16, L.ln1_w, L.ln1_b, eps, nullptr, b.H, Xc, mc, D, s, keep1));
        else IISAN_TRY(launch_add_layernorm768(dt, Xc, b.D16, L.ln2_w, L.ln2_b, eps, Xc, b.H, nullptr, mc, D, s));
        IISAN_TRY(launch(plain(fc1_mode(), D, F, mc), b.H, L.fc1_w, L.fc1_b, b.F1));
        IISAN_TRY(launch(plain(EPI_OUT16, F, D, mc), b.F1, L.fc2_w, L.fc2_b, b.D16));
        if (post_ln) IISAN_TRY(launch_add_layernorm768(dt, Xc, b.D16, L.ln2_w, L.ln2_b, eps, nullptr, nullptr, Xc, mc, D, s, keep2));
        else IISAN_TRY(launch_add_layernorm768(dt, Xc, b.D16, nullptr, nullptr, eps, Xc, nullptr, nullptr, mc, D, s));
        return launch_gather_cls(Xc, tp, mc, 1, D, n_taps, k, s);
    }
};

}  // namespace

IISAN_DEV_KNOB(full_blocks, g_full_blocks);
IISAN_DEV_KNOB(resid32, g_resid32);
IISAN_DEV_KNOB(ln_fold, g_ln_fold);
IISAN_DEV_KNOB(blk32, g_blk32);
static int vit_fold_layers(const iisan_vit_weights* w) {
    return (!g_resid32 && g_ln_fold && vit_fold_routes(w->dtype16, w->hidden, vit_is_clip(w))) ? w->layers : 0;
}
// the folded set of one tower: [layers][(3D + F) x D] fp16, then [layers][3D + F] fp32 (the caller's `folded` buffer or the workspace)
static size_t vit_fold_w_elems(const iisan_vit_weights* w) { return (size_t)(3 * w->hidden + w->mlp) * w->hidden; }
static int vit_fold_all(const iisan_vit_weights* w, int layers, bool last_fc1, char* Wf, float* Bf, hipStream_t s) {
    const int D = w->hidden, F = w->mlp;
    LnFoldJob jobs[32];
    int nj = 0;
    for (int l = 0; l < layers; ++l) {
        const iisan_layer_weights& L = w->layer[l];
        char* wq = Wf + (size_t)l * vit_fold_w_elems(w) * 2;
        float* bq = Bf + (size_t)l * (3 * D + F);
        jobs[nj++] = LnFoldJob{L.qkv_w32 ? (const void*)L.qkv_w32 : L.qkv_w, L.qkv_b, L.ln1_w, L.ln1_b, wq, bq, 3 * D, L.qkv_w32 ? 1 : 0};
        if (l + 1 < layers || last_fc1)
            jobs[nj++] = LnFoldJob{L.fc1_w32 ? (const void*)L.fc1_w32 : L.fc1_w, L.fc1_b, L.ln2_w, L.ln2_b, wq + (size_t)3 * D * D * 2, bq + 3 * D, F, L.fc1_w32 ? 1 : 0};
        if (nj >= 31 || l + 1 == layers) { IISAN_TRY(launch_fold_ln_weights(jobs, nj, s)); nj = 0; }
    }
    return IISAN_OK;
}

extern "C" size_t iisan_vit_fold_bytes(const iisan_vit_weights* w) {
    if (!vit_fold_routes(w->dtype16, w->hidden, vit_is_clip(w))) return 0;
    return (size_t)w->layers * (vit_fold_w_elems(w) * 2 + (size_t)(3 * w->hidden + w->mlp) * 4);
}

extern "C" int iisan_vit_fold_layernorm(const iisan_vit_weights* w, void* folded, size_t bytes, void* stream) {
    const size_t need = iisan_vit_fold_bytes(w);
    IISAN_CHECK_SHAPE(need > 0, "vit_fold_layernorm: fp16 operands and hidden size 768 only, and no CLIP tower");
    if (!folded || bytes < need) {
        iisan_set_error("vit_fold_layernorm: buffer too small (%zu < %zu)", bytes, need);
        return IISAN_EWORKSPACE;
    }
    IISAN_CHECK_SHAPE(w->layers >= 1 && w->layers <= IISAN_MAX_LAYERS, "vit_fold_layernorm: layers %d out of range", w->layers);
    return vit_fold_all(w, w->layers, true, (char*)folded, (float*)((char*)folded + (size_t)w->layers * vit_fold_w_elems(w) * 2), (hipStream_t)stream);
}

// the workspace of a ViT call that runs in chunks of Mc items (c.off: its size)
static void vit_carve(WsCarver& c, EncBufs& b, const iisan_vit_weights* w, int64_t Mc) {
    const int P = (w->image / w->patch) * (w->image / w->patch);
    const int pd = vit_patch_ld(w->channels, w->patch);
    carve(c, b, Mc * (P + 1), Mc, w->hidden, w->mlp > pd ? w->mlp : pd, 0, vit_fold_layers(w), w->folded == nullptr);
}

extern "C" size_t iisan_vit_forward_taps_ws_bytes(const iisan_vit_weights* w, int64_t M, int64_t chunk_items) {
    WsCarver c(nullptr, 0);
    EncBufs b;
    vit_carve(c, b, w, Chunks(M, chunk_items).Mc);
    return c.off;
}

namespace {

// How one call carries the residual stream of the pre-LN tower; decided once per call (vit_plan).  Each strategy is three steps of
// VitChunk (VIT_STEPS): `open` (the stream becomes hidden state l; LN1), `mid` (between the O and the FC1 product of an all-token block:
// LN2) and `close` (the last hidden state, when it is tapped).  The products around them are those of Products under the strategy's flags.
enum VitStrategy {
    VS_RESID32,     // dev knob resid32: the whole stream fp32 in X, LayerNorm images in H
    VS_IMAGE,       // mixed stream (fp16 rows in X16, fp32 CLS rows in Xc), LayerNorm images in H: ln_fold = 0, bf16 operands, small batches
    VS_FOLD,        // mixed stream, no image: the add kernels leave rstd per row, the QKV / FC1 products apply LayerNorm (ln_fold = 1)
    VS_STREAM,      // ... and no add kernels: the O / FC2 products add into the stream in their epilogues (ln_fold = 2, the product route)
};
struct VitPlan {
    VitStrategy st;
    bool folds;     // the call folds the LayerNorms into the weights itself (the weights struct carries no folded set)
};

// The strategy and the two layouts of a ViT call, left in p.  LayerNorm in the epilogues of the QKV / FC1 products (g_ln_fold) only where
// those products run on the kernel that has it, and the residual adds in the epilogues of the O / FC2 products likewise.  The stream is
// block-major only on the product route, with F1 block-major, and only when every product that touches it takes the flags: QKV and FC1 (A),
// O and FC2 (read-modify-write), the K/V product of a CLS-only last block (A).
VitPlan vit_plan(Products& p, int live, bool full_blocks, bool folded, const Chunks& c, bool clip) {
    if (g_resid32) return {VS_RESID32, false};
    const int reads = Products::P_QKV | Products::P_FC1 | (full_blocks ? 0 : Products::P_KV), adds = Products::P_O | Products::P_FC2;
    Products t = p;
    t.ln = true;
    if (live > 0 && g_ln_fold && vit_fold_routes(p.dt, p.D, clip) && t.all_h256(c, reads)) {
        p = t;
        t.stream = true;
        if (g_ln_fold >= 2 && t.all_h256(c, adds)) p = t;
    }
    t = p;
    t.f1blk = t.xblk = true;
    if (g_blk32 >= 2 && p.stream && t.all_h256(c, reads | adds)) p = t;
    else p.f1blk = p.f1_blk32(c);
    const VitStrategy st = !p.ln ? VS_IMAGE : p.stream ? VS_STREAM : VS_FOLD;
    return {st, st >= VS_FOLD && !folded};
}

constexpr int MX_ADD_STAT = MX_D1 | MX_RESV | MX_STAT;       // x += d (fp16 stream, fp32 CLS rows); row statistics

// One chunk of a ViT forward.
// The O / FC2 products of resid32 / image / fold emit 16-bit DELTAS (dO in D16, dF in D16b); the residual add is fused into a later
// LayerNorm kernel (HBM-bound) instead of a read-modify-write GEMM epilogue.  Pre-LN tower, resid32 / image: LN2 computes LN(x + dO)
// WITHOUT writing x back; the next open step adds both deltas, (x + dO) + dF in fp32 — the same value — and writes x once per block
// instead of twice.
struct VitChunk : Chunk {
    const iisan_vit_weights* w;

    const iisan_layer_weights& layer(int l) const { return w->layer[l]; }
    // the folded set of layer l (vit_fold_all)
    char* Wf_qkv(int l) const { return (char*)b.Wf + (size_t)l * (3 * D + F) * D * 2; }
    char* Wf_fc1(int l) const { return Wf_qkv(l) + (size_t)3 * D * D * 2; }
    float* bf_qkv(int l) const { return b.Bf + (size_t)l * (3 * D + F); }
    float* bf_fc1(int l) const { return bf_qkv(l) + 3 * D; }

    // index != null: `img` is a resident uint8 catalogue of `rows` images and item m of the chunk is its row index[m]
    int embed(const void* img, int img_u8, const int64_t* index = nullptr, int64_t rows = 0) const {
        const int P = T - 1, pd = vit_patch_ld(w->channels, w->patch);      // (588 -> 640 columns at patch 14: zeros in F1 and in patch_w)
        // per-channel statistics of a uint8 source (mean | std are adjacent in the struct); all zero: the reference's transform, the launch as it was
        bool nz = false;
        for (int c = 0; c < 3; ++c) nz = nz || w->norm_mean[c] != 0.f || w->norm_std[c] != 0.f;
        const float norm6[6] = {w->norm_mean[0], w->norm_mean[1], w->norm_mean[2], w->norm_std[0], w->norm_std[1], w->norm_std[2]};
        const float* norm = nz && img_u8 ? norm6 : nullptr;
        if (index) IISAN_TRY(launch_vit_im2col_indexed(dt, (const uint8_t*)img, rows, index, b.F1, mc, w->channels, w->image, w->patch, s, norm));
        else IISAN_TRY(launch_vit_im2col(dt, img, img_u8, b.F1, mc, w->channels, w->image, w->patch, s, norm));
        // patch embedding: resid32 = fp32 token rows with the position embedding added (128x128 kernel); mixed = 16-bit rows on the
        // production GEMM (gemm16_h256, 0.40 against 0.59 ms at bs = 128), the position table is added by block 0's open step
        Product pe = patch(!mixed, pd, D, mc * P, P);
        pe.a.pos = mixed ? nullptr : w->pos_emb;
        IISAN_TRY(launch(pe, b.F1, w->patch_w, w->patch_b, mixed ? b.D16b : (void*)b.X));
        // CLS rows: cls + pos[0] — into the fp32 stream (token-major) or into the compact fp32 CLS stream
        return launch_vit_cls_rows(mixed ? b.Xc : b.X, w->cls_token, w->pos_emb, mc, mixed ? 1 : T, D, s);
    }
    // CLIP, a call that taps hidden state 0 alone (no block runs, so no open step): block 0's open step all the same — the kernel every
    // other call gets hidden state 0 from, so that tap 0 has the same bits whichever taps are asked for
    int pre_ln_only() const { return mixed ? open_image(0) : open_resid32(0); }
    // ---- VS_RESID32 ------------------------------------------------------------------------------------------------------------
    int open_resid32(int l) const {     // x += dO + dF of block l - 1 ; h = LN1(x)
        const iisan_layer_weights& L = layer(l);
        // (CLIP under the dev switch: the pre-LayerNorm in place, a launch of its own — the one-pass opening kernel is the mixed stream's)
        if (l == 0 && w->pre_ln_w) IISAN_TRY(launch_layernorm768(dt, b.X, w->pre_ln_w, w->pre_ln_b, eps, nullptr, b.X, tok, D, s));
        if (l == 0) return launch_add2_layernorm768(dt, b.X, nullptr, nullptr, L.ln1_w, L.ln1_b, eps, nullptr, b.H, nullptr, tok, D, s);
        return launch_add2_layernorm768(dt, b.X, b.D16, b.D16b, L.ln1_w, L.ln1_b, eps, b.X, b.H, nullptr, tok, D, s);
    }
    // h = LN2(x + dO)   (x itself is updated by the next open step)
    int mid_resid32(int l) const { return launch_add_layernorm768(dt, b.X, b.D16, layer(l).ln2_w, layer(l).ln2_b, eps, nullptr, b.H, nullptr, tok, D, s); }
    int close_resid32() const { return launch_add2_layernorm768(dt, b.X, b.D16, b.D16b, nullptr, nullptr, eps, b.X, nullptr, nullptr, tok, D, s); }

    // ---- VS_IMAGE ----------------------------------------------------------------------------------------------------------------
    int open_image(int l) const {
        const iisan_layer_weights& L = layer(l);
        if (l == 0 && w->pre_ln_w)      // CLIP: ... -> pre-LayerNorm -> stream (fp16 rows, fp32 CLS rows: hidden state 0) + LN image, one launch
            return launch_clip_open(dt, w->pos_emb, b.X16, b.Xc, b.D16b, w->pre_ln_w, w->pre_ln_b, L.ln1_w, L.ln1_b, eps, b.H, mc, T, D, s);
        if (l == 0)     // position table + 16-bit patch embedding -> fp16 stream of the patch rows (the CLS rows are in Xc already) + LN image
            return launch_layernorm768_mixed(dt, MX_SRC32 | MX_POSROW | MX_D1 | MX_RESV | MX_LN, w->pos_emb, b.X16, b.Xc, b.D16b, nullptr, L.ln1_w, L.ln1_b, eps, b.H, mc, T, D, s);
        return launch_layernorm768_mixed(dt, MX_D1 | MX_D2 | MX_RESV | MX_LN, nullptr, b.X16, b.Xc, b.D16, b.D16b, L.ln1_w, L.ln1_b, eps, b.H, mc, T, D, s);
    }
    // h = LN2(x + dO)   (x itself is updated by the next open step)
    int mid_image(int l) const { return launch_layernorm768_mixed(dt, MX_D1 | MX_LN, nullptr, b.X16, b.Xc, b.D16, nullptr, layer(l).ln2_w, layer(l).ln2_b, eps, b.H, mc, T, D, s); }
    // only the CLS rows of the last hidden state are consumed
    int close_image() const { return launch_layernorm768_mixed(dt, MX_D1 | MX_D2 | MX_RESV | MX_CLSONLY, nullptr, b.X16, b.Xc, b.D16, b.D16b, nullptr, nullptr, eps, nullptr, mc, T, D, s); }

    // ---- VS_FOLD: the stream + rstd per row; LN1 / LN2 are applied by the epilogues of the QKV / FC1 products -------------------------
    int patches_to_stream() const {     // position table + 16-bit patch embedding -> fp16 stream of the patch rows (the CLS rows are in Xc already)
        return launch_layernorm768_mixed(dt, MX_SRC32 | MX_POSROW | MX_ADD_STAT | (xblk ? MX_BLK32 : 0), w->pos_emb, b.X16, b.Xc, b.D16b, nullptr, nullptr, nullptr, eps, nullptr, mc, T, D, s, b.RS);
    }
    // x += d in the stream; rstd of the new rows
    int add_stat(const void* d) const { return launch_layernorm768_mixed(dt, MX_ADD_STAT, nullptr, b.X16, b.Xc, d, nullptr, nullptr, nullptr, eps, nullptr, mc, T, D, s, b.RS); }
    // x += dF of block l - 1 (x + dO is in the stream already: that block wrote it in its mid step)
    int open_fold(int l) const { return l == 0 ? patches_to_stream() : add_stat(b.D16b); }
    // x += dO (written: the FC1 product reads the stream); LN2 in the FC1 product's epilogue
    int mid_fold(int) const { return add_stat(b.D16); }
    // x + dO is in the stream: the CLS rows take dF
    int close_fold() const { return launch_layernorm768_mixed(dt, MX_D1 | MX_RESV | MX_CLSONLY, nullptr, b.X16, b.Xc, b.D16b, nullptr, nullptr, nullptr, eps, nullptr, mc, T, D, s); }

    // ---- VS_STREAM: ... and the O / FC2 products add into the stream and leave its row statistics: no step but the first ------------------
    int open_stream(int l) const { return l == 0 ? patches_to_stream() : IISAN_OK; }
    int mid_stream(int) const { return IISAN_OK; }
    int close_stream() const { return IISAN_OK; }       // the stream is the last hidden state already

    // ---- the blocks: every product as Products describes it under the strategy ------------------------------------------------------------
    // the A operand of the QKV / FC1 products: the LayerNorm image against the tower's weights, or the stream itself against the folded set
    const void* act() const { return ln ? b.X16 : b.H; }
    // an O / FC2 product: its 16-bit delta into `d`; VS_STREAM: x += A W^T + bias in the stream instead (fp16 rows in place, the CLS rows'
    // fp32 stream through the finalize step) and rstd of the new rows
    int delta(const Product& p, const void* A, const void* W, const float* bias, void* d) const {
        if (!stream) return launch(p, A, W, bias, d);
        IISAN_TRY(launch(p, A, W, bias, b.X16));
        return launch_stream_stats_finalize(b.RP, D / 64, ceil_div(tok, 256) * 256, b.X16, b.Xc, b.RS, eps, mc, T, s, xblk);
    }
    int full_block(int l, int (VitChunk::*mid)(int) const) const {
        const iisan_layer_weights& L = layer(l);
        IISAN_TRY(launch(qkv(tok), act(), ln ? Wf_qkv(l) : L.qkv_w, ln ? bf_qkv(l) : L.qkv_b, b.QKV));
        if (hd80()) IISAN_TRY(launch_attention16_hd80(dt, b.QKV, nullptr, b.H, mc, T, heads, s));
        else IISAN_TRY(launch_attention16(dt, b.QKV, nullptr, b.H, mc, T, heads, s));
        IISAN_TRY(delta(o(tok), b.H, L.o_w, L.o_b, b.D16));
        IISAN_TRY((this->*mid)(l));
        IISAN_TRY(launch(fc1(tok), act(), ln ? Wf_fc1(l) : L.fc1_w, ln ? bf_fc1(l) : L.fc1_b, b.F1));
        return delta(fc2(tok), b.F1, L.fc2_w, L.fc2_b, b.D16b);
    }
    // the CLS-only last live block (Chunk::cls_tail); its output goes to tap k
    int cls_block(int l, int k) const {
        // the K / V product, the CLS attention kernel and the CLS tail are written for 64-wide heads: the executor runs the last live block of an
        // 80-wide-head tower on every token and never comes here
        IISAN_CHECK_SHAPE(!hd80(), "vit: no CLS-only form of the last live block for 80-wide heads (hidden %d, heads %d)", D, heads);
        const iisan_layer_weights& L = layer(l);
        // the CLS rows' LN1 image: from their fp32 stream, or gathered from the image of every row
        if (ln) IISAN_TRY(launch_layernorm768(dt, b.Xc, L.ln1_w, L.ln1_b, eps, b.Cls, nullptr, mc, D, s));
        else IISAN_TRY(launch_gather_rows16(b.H, b.Cls, mc, T, D, s));
        // K / V of every token (ln: from the stream, LN1 in the epilogue): the last two thirds of the QKV weights
        IISAN_TRY(launch(qkv(tok, 1), act(), (ln ? Wf_qkv(l) : (const char*)L.qkv_w) + (size_t)D * D * 2, (ln ? bf_qkv(l) : L.qkv_b) + D, b.QKV));
        return cls_tail(L, nullptr, nullptr, false, nullptr, nullptr, k);
    }
};

// the three steps of every strategy, indexed by VitStrategy
const struct { int (VitChunk::*open)(int) const; int (VitChunk::*mid)(int) const; int (VitChunk::*close)() const; } VIT_STEPS[] = {
    {&VitChunk::open_resid32, &VitChunk::mid_resid32, &VitChunk::close_resid32},
    {&VitChunk::open_image, &VitChunk::mid_image, &VitChunk::close_image},
    {&VitChunk::open_fold, &VitChunk::mid_fold, &VitChunk::close_fold},
    {&VitChunk::open_stream, &VitChunk::mid_stream, &VitChunk::close_stream},
};

}  // namespace

// index != null: `images` is a resident uint8 catalogue [rows, C, R, R] and slot m reads row index[m] (the chunk loop offsets the
// index, never the catalogue)
static int vit_forward_taps_impl(const iisan_vit_weights* w, const void* images, int img_u8, int64_t M,
                                 const int32_t* tap_layers, int32_t n_taps, float* taps, int64_t chunk_items,
                                 void* ws, size_t ws_bytes, void* stream, const int64_t* index = nullptr, int64_t rows = 0) {
    hipStream_t s = (hipStream_t)stream;
    IISAN_CHECK_SHAPE(M > 0, "vit_forward_taps: M must be positive");
    IISAN_TRY(check_common(true, w->hidden, w->layers, w->heads, w->mlp, n_taps, tap_layers));
    // patch sides: the multiples of 8, and 14 (ViT-H/14) through the padded patch extraction
    IISAN_CHECK_SHAPE((w->patch % 8 == 0 || w->patch == 14) && w->patch > 0 && w->image % w->patch == 0, "vit: patch %d / image %d unsupported", w->patch, w->image);
    const int D = w->hidden, T = (w->image / w->patch) * (w->image / w->patch) + 1;
    // a patch side that is a multiple of 8 takes its patch vector as it is; 14 is zero-padded to a multiple of 64 by the patch
    // extraction, and patch_w carries the same padding (vit_patch_ld)
    const int pd = vit_patch_ld(w->channels, w->patch);
    IISAN_CHECK_SHAPE(pd % 64 == 0, "vit: patch vector length %d must be a multiple of 64", pd);
    IISAN_TRY(vit_check_tokens(T));
    const Chunks c(M, chunk_items);
    WsCarver cv(ws, ws_bytes);
    EncBufs b;
    vit_carve(cv, b, w, c.Mc);
    if (w->folded && b.RS) {       // the caller folded once (iisan_vit_fold_layernorm)
        b.Wf = const_cast<void*>(w->folded);
        b.Bf = (float*)((char*)b.Wf + (size_t)w->layers * vit_fold_w_elems(w) * 2);
    }
    if (cv.overflow || !ws) {
        iisan_set_error("vit_forward_taps: workspace too small (%zu < %zu)", ws_bytes, cv.off);
        return IISAN_EWORKSPACE;
    }
    const bool full_blocks = g_full_blocks || w->full_blocks;
    // Blocks after the deepest tapped hidden state are dead code (Versa configurations tap a prefix of the tower)
    const int live = full_blocks ? w->layers : max_tap(tap_layers, n_taps);
    // a CLIP tower: a LayerNorm in front of block 0 and / or quick-GELU in the MLP
    IISAN_CHECK_SHAPE(!w->pre_ln_w == !w->pre_ln_b, "vit: pre_ln_w and pre_ln_b come together (one of them is null)");
    IISAN_CHECK_SHAPE(w->act == 0 || w->act == 1, "vit: activation %d is neither erf-GELU (0) nor quick-GELU (1)", w->act);
    const bool pre = w->pre_ln_w != nullptr;
    Products p{w->dtype16, D, w->mlp, T, w->heads, w->act};
    // 80-wide heads: the last live block has no CLS-only form and runs on every token (1 / 32 of a ViT-H)
    const bool all_tokens = full_blocks || p.hd80();
    const VitPlan plan = vit_plan(p, live, all_tokens, w->folded != nullptr, c, vit_is_clip(w));
    const auto& step = VIT_STEPS[plan.st];
    if (plan.folds) IISAN_TRY(vit_fold_all(w, live, full_blocks, (char*)b.Wf, b.Bf, s));
    const int64_t img_elems = (int64_t)w->channels * w->image * w->image;
    for (int64_t m0 = 0; m0 < M; m0 += c.Mc) {
        const int64_t mc = (M - m0 < c.Mc) ? M - m0 : c.Mc;
        const VitChunk ch{{p, b, s, w->eps, plan.st != VS_RESID32, m0, mc, mc * T, taps + m0 * n_taps * D, n_taps}, w};
        if (index) IISAN_TRY(ch.embed(images, 1, index + m0, rows));
        else IISAN_TRY(ch.embed(img_u8 ? (const void*)((const uint8_t*)images + m0 * img_elems) : (const void*)((const float*)images + m0 * img_elems), img_u8));
        // hidden state 0: the embeddings — or, with a pre-LayerNorm, its output, which block 0's open step leaves in the stream
        int k = tap_index(tap_layers, n_taps, 0);
        if (k >= 0 && pre && live == 0) IISAN_TRY(ch.pre_ln_only());
        if (k >= 0 && !(pre && live > 0)) IISAN_TRY(ch.tap(k));
        for (int l = 0; l < live; ++l) {
            IISAN_TRY((ch.*step.open)(l));       // -> the stream is hidden state l
            k = tap_index(tap_layers, n_taps, l);
            if (k >= 0 && (l > 0 || pre)) IISAN_TRY(ch.tap(k));
            if (l + 1 < live || all_tokens) IISAN_TRY(ch.full_block(l, step.mid));
            else IISAN_TRY(ch.cls_block(l, tap_index(tap_layers, n_taps, live)));
        }
        // (full_blocks: live = the whole tower.  live = 0: no block has run, tap 0 is written above and there is nothing to close)
        k = all_tokens && live > 0 ? tap_index(tap_layers, n_taps, live) : -1;
        if (k >= 0) {
            IISAN_TRY((ch.*step.close)());
            IISAN_TRY(ch.tap(k));
        }
    }
    return IISAN_OK;
}

extern "C" int iisan_vit_forward_taps(const iisan_vit_weights* w, const float* images, int64_t M,
                                      const int32_t* tap_layers, int32_t n_taps, float* taps, int64_t chunk_items,
                                      void* ws, size_t ws_bytes, void* stream) {
    return vit_forward_taps_impl(w, images, 0, M, tap_layers, n_taps, taps, chunk_items, ws, ws_bytes, stream);
}

extern "C" int iisan_vit_forward_taps_u8(const iisan_vit_weights* w, const uint8_t* images, int64_t M,
                                         const int32_t* tap_layers, int32_t n_taps, float* taps, int64_t chunk_items,
                                         void* ws, size_t ws_bytes, void* stream) {
    IISAN_CHECK_SHAPE(w->image % 8 == 0, "vit u8: image side %d must be a multiple of 8", w->image);
    return vit_forward_taps_impl(w, images, 1, M, tap_layers, n_taps, taps, chunk_items, ws, ws_bytes, stream);
}

extern "C" int iisan_vit_forward_taps_u8_indexed(const iisan_vit_weights* w, const uint8_t* catalogue, int64_t rows,
                                                 const int64_t* index, int64_t M, const int32_t* tap_layers, int32_t n_taps,
                                                 float* taps, int64_t chunk_items, void* ws, size_t ws_bytes, void* stream) {
    IISAN_CHECK_SHAPE(rows > 0, "vit u8 indexed: the catalogue needs at least one row (rows = %lld)", (long long)rows);
    IISAN_CHECK_SHAPE(catalogue != nullptr && index != nullptr, "vit u8 indexed: null %s", catalogue ? "index" : "catalogue");
    IISAN_CHECK_SHAPE(w->image % 8 == 0, "vit u8 indexed: image side %d must be a multiple of 8", w->image);
    IISAN_CHECK_SHAPE(M > 0, "vit u8 indexed: M must be positive");
    return vit_forward_taps_impl(w, catalogue, 1, M, tap_layers, n_taps, taps, chunk_items, ws, ws_bytes, stream, index, rows);
}

// ---- DeBERTa: the projected position tables (include/iisan_hip.h, iisan_deberta_rel_project) ---------------------------------------------------
// one layer's image: [heads][3][2 span][64] 16-bit elements = 3 * 2 span * D
static size_t deberta_rel_layer_elems(const iisan_bert_weights* w) { return (size_t)3 * 2 * w->span * w->hidden; }
static bool bert_is_deberta(const iisan_bert_weights* w) { return w->rel_emb != nullptr; }
static int deberta_check_span(int span) {
    IISAN_CHECK_SHAPE(span >= 1 && span <= 256, "deberta: span (position_buckets) %d outside 1 .. 256", span);
    return IISAN_OK;
}
// the titles the identity part of HF's log-bucket map covers (|i - j| <= span / 2), and what attn16_disent.hip keeps in LDS
static int deberta_check_words(int words, int span) {
    IISAN_CHECK_SHAPE(words <= span / 2, "deberta: %d words > span / 2 = %d: relative positions past position_buckets / 2 fall into HF's log "
                      "buckets, which this tower does not implement", words, span / 2);
    IISAN_CHECK_SHAPE(words <= 128, "deberta: %d words > 128 not supported", words);
    return IISAN_OK;
}

extern "C" size_t iisan_deberta_rel_bytes(const iisan_bert_weights* w) {
    return bert_is_deberta(w) && w->span > 0 && w->layers > 0 ? (size_t)w->layers * deberta_rel_layer_elems(w) * 2 : 0;
}
// the 16-bit LayerNorm image of the table, rows padded to a GEMM row tile
extern "C" size_t iisan_deberta_rel_ws_bytes(const iisan_bert_weights* w) {
    return bert_is_deberta(w) && w->span > 0 ? align_up((size_t)ceil_div(2 * w->span, 256) * 256 * w->hidden * 2, 256) : 0;
}
// tables of layers 0 .. layers - 1 into `out`: LayerNorm of the table by the row kernel, then per layer ONE product with the layer's own QKV
// matrix through the head-major epilogue — the table is a pseudo-item of 2 span tokens
static int deberta_rel_project(const iisan_bert_weights* w, int layers, void* out, void* ws, hipStream_t s) {
    const int D = w->hidden, R = 2 * w->span;
    IISAN_TRY(launch_layernorm768(w->dtype16, w->rel_emb, w->rel_ln_w, w->rel_ln_b, w->eps, ws, nullptr, R, D, s));
    for (int l = 0; l < layers; ++l) {
        Gemm16Args a{};
        a.A = ws; a.W = w->layer[l].qkv_w; a.bias = w->layer[l].qkv_b; a.out = (char*)out + (size_t)l * deberta_rel_layer_elems(w) * 2;
        a.M = R; a.N = 3 * D; a.K = D; a.lda = D; a.ldw = D; a.ldo = 3 * D;
        a.qkv_S = R; a.qkv_heads = w->heads; a.qkv_which0 = 0;
        IISAN_TRY(launch_gemm16(w->dtype16, EPI_QKVH16, a, s));
    }
    return IISAN_OK;
}
static int deberta_check_struct(const iisan_bert_weights* w) {
    IISAN_CHECK_SHAPE(w->rel_emb && w->rel_ln_w && w->rel_ln_b, "deberta: rel_emb, rel_ln_w and rel_ln_b come together (one of them is null)");
    IISAN_CHECK_SHAPE(!w->pos_emb && !w->type_emb, "deberta: a tower with rel_emb has no position and no type table (pos_emb / type_emb must be null)");
    return deberta_check_span(w->span);
}
extern "C" int iisan_deberta_rel_project(const iisan_bert_weights* w, void* out, void* ws, size_t ws_bytes, void* stream) {
    IISAN_TRY(deberta_check_struct(w));
    IISAN_CHECK_SHAPE(row_width_instantiated(w->hidden) && w->hidden != 1280 && w->heads > 0 && w->hidden == w->heads * 64,
                      "deberta_rel_project: hidden %d / heads %d not supported", w->hidden, w->heads);
    IISAN_CHECK_SHAPE(w->layers >= 1 && w->layers <= IISAN_MAX_LAYERS, "deberta_rel_project: layers %d out of range", w->layers);
    const size_t need = iisan_deberta_rel_ws_bytes(w);
    if (!out || !ws || ws_bytes < need) {
        iisan_set_error("deberta_rel_project: null output or workspace too small (%zu < %zu)", ws_bytes, need);
        return IISAN_EWORKSPACE;
    }
    return deberta_rel_project(w, w->layers, out, ws, (hipStream_t)stream);
}

// the workspace of a BERT call in chunks of Mc items; a DeBERTa struct without rel_proj: + the projected tables and their scratch
static size_t bert_carve(WsCarver& c, EncBufs& b, const iisan_bert_weights* w, int64_t Mc, int words, void** rel, void** rel_ws) {
    carve(c, b, Mc * words, Mc, w->hidden, w->mlp, Mc * words);
    *rel = *rel_ws = nullptr;
    if (bert_is_deberta(w) && !w->rel_proj) {
        *rel = c.take<uint8_t>(iisan_deberta_rel_bytes(w));
        *rel_ws = c.take<uint8_t>(iisan_deberta_rel_ws_bytes(w));
    }
    return c.off;
}

extern "C" size_t iisan_bert_forward_taps_ws_bytes(const iisan_bert_weights* w, int64_t M, int32_t words, int64_t chunk_items) {
    const int64_t Mc = Chunks(M, chunk_items).Mc;
    WsCarver c(nullptr, 0);
    EncBufs b;
    void *rel, *rel_ws;
    return bert_carve(c, b, w, Mc, words, &rel, &rel_ws);
}

namespace {

// What a BERT call decides before its first launch, beside p.f1blk.  Post-LN tower: the stream IS the LayerNorm output.  resid32: X fp32
// [tok, D]; mixed: Xc fp32 (CLS rows) + X16 fp16.  alias: with fp16 operands the 16-bit image the products read and the fp16 stream are the same
// values: one buffer, written once (g_ln_fold; the add + LayerNorm kernels move 6 instead of 8 bytes per element)
struct BertPlan { bool mixed, alias; };
BertPlan bert_plan(Products& p, const Chunks& c) {
    p.f1blk = p.f1_blk32(c);
    const bool mixed = !g_resid32;
    return {mixed, mixed && p.dt == IISAN_F16 && g_ln_fold != 0};
}

// One chunk of a BERT forward.  Eval mode (dropping = false) is the launch sequence below with null keeps; in train mode the attention kernel of
// bert_drop.hip takes the place of the eval-mode one, and the embedding and add + LayerNorm steps run their train-mode instantiations (a RowKeep
// instead of null; rowops.hip) — sites 0, 1 + 3l, 2 + 3l, 3 + 3l and their indices: include/iisan_hip.h, iisan_bert_dropout
// kind: IISAN_TOWER_BERT, or IISAN_TOWER_DEBERTA — the same block skeleton with three steps switched: the embedding (no position / type table, the
// mask multiply), the attention of an all-token block and the attention of the CLS tail (disentangled, over `rel`, the projected tables of
// every layer).  Eval mode only.
struct BertChunk : Chunk {
    const iisan_bert_weights* w; bool alias, dropping; float hp, ap; uint64_t seed;
    int kind = IISAN_TOWER_BERT; const void* rel = nullptr;

    bool deberta() const { return kind == IISAN_TOWER_DEBERTA; }
    const void* rel_layer(int l) const { return (const char*)rel + (size_t)l * deberta_rel_layer_elems(w) * 2; }

    void* img() const { return alias ? b.X16 : b.H; }       // the 16-bit image of the stream: the A operand of the QKV / FC1 products
    // train mode: the keep functor of a hidden site, local row r of the launch = token row m0 * T + r * rs of the whole call (rs = 1: the rows of
    // the chunk; rs = T: compact CLS rows, the masks of token row t = 0 of the all-token execution); eval: null
    struct Keep {
        RowKeep rk; bool on;
        operator const RowKeep*() const { return on ? &rk : nullptr; }
    };
    Keep keep(int site, int rs) const { return {RowKeep{make_drop(seed, site, hp), m0 * T, rs}, dropping}; }
    DropCfg attn_drop(int l) const { return make_drop(seed, 1 + 3 * l, ap); }

    // index != null: `text` is a resident table [rows, 2W] and item m of the chunk is its row index[m0 + m]
    int embed(const int64_t* text, const int64_t* index, int64_t rows) const {
        const Keep k = keep(0, 1);
        // (DeBERTa: pos_emb and type_emb are null — the launchers' DeBERTa instantiation, LayerNorm(word[id]) * mask)
        if (index) return launch_bert_embed_ln_indexed(dt, text, rows, index + m0, w->word_emb, w->pos_emb, w->type_emb, w->emb_ln_w, w->emb_ln_b, w->eps,
                                                       mixed ? nullptr : b.X, img(), b.KB, mc, T, w->vocab, D, s, b.X16, b.Xc, k);
        return launch_bert_embed_ln(dt, text + m0 * 2 * T, w->word_emb, w->pos_emb, w->type_emb, w->emb_ln_w, w->emb_ln_b, w->eps,
                                    mixed ? nullptr : b.X, img(), b.KB, mc, T, w->vocab, D, s, b.X16, b.Xc, k);
    }
    // x = LN(x + delta): stream and 16-bit image out
    int add_ln(const float* g, const float* be, int site) const {
        const Keep k = keep(site, 1);
        return mixed ? launch_layernorm768_mixed(dt, MX_D1 | MX_LN | MX_RESY | (alias ? MX_ALIAS : 0), nullptr, b.X16, b.Xc, b.D16, nullptr, g, be, eps, img(), mc, T, D, s, nullptr, k)
                     : launch_add_layernorm768(dt, b.X, b.D16, g, be, eps, nullptr, b.H, b.X, tok, D, s);
    }
    int full_block(int l) const {
        const iisan_layer_weights& L = w->layer[l];
        // a = LN(x + O(attn(x)))
        IISAN_TRY(launch(qkv(tok), img(), L.qkv_w, L.qkv_b, b.QKV));
        if (deberta()) IISAN_TRY(launch_attention16_disent(dt, b.QKV, rel_layer(l), b.KB, b.H, mc, T, heads, w->span, s));
        else if (dropping) IISAN_TRY(launch_attention16_drop(dt, b.QKV, b.KB, b.H, mc, T, heads, attn_drop(l), m0, false, nullptr, s));
        else IISAN_TRY(launch_attention16(dt, b.QKV, b.KB, b.H, mc, T, heads, s));
        IISAN_TRY(launch(o(tok), b.H, L.o_w, L.o_b, b.D16));
        IISAN_TRY(add_ln(L.ln1_w, L.ln1_b, 2 + 3 * l));
        // x = LN(a + FC2(gelu(FC1 a)))
        IISAN_TRY(launch(fc1(tok), img(), L.fc1_w, L.fc1_b, b.F1));
        IISAN_TRY(launch(fc2(tok), b.F1, L.fc2_w, L.fc2_b, b.D16));
        return add_ln(L.ln2_w, L.ln2_b, 3 + 3 * l);
    }
    // the CLS-only last live block (Chunk::cls_tail).  Post-LN tower: the block input is the 16-bit image of x, so its CLS rows are gathered directly
    int cls_block(int l, int k) const {
        const iisan_layer_weights& L = w->layer[l];
        IISAN_TRY(launch_gather_rows16(img(), b.Cls, mc, T, D, s));
        IISAN_TRY(launch(qkv(tok, 1), img(), (const char*)L.qkv_w + (size_t)D * D * 2, L.qkv_b + D, b.QKV));
        const DropCfg ad = attn_drop(l);
        const Keep k1 = keep(2 + 3 * l, T), k2 = keep(3 + 3 * l, T);
        return cls_tail(L, b.KB, dropping ? &ad : nullptr, true, k1, k2, k, deberta() ? rel_layer(l) : nullptr, w->span);
    }
};

}  // namespace

// index != null: `text` is a resident table [rows, 2W] and slot m reads row index[m] (the chunk loop offsets the index, never the table)
// drop: null or both probabilities 0 = eval mode; otherwise train mode (BertChunk)
static int bert_forward_taps_impl(const iisan_bert_weights* w, const int64_t* text, int64_t M, int32_t words,
                                  const int32_t* tap_layers, int32_t n_taps, float* taps, int64_t chunk_items,
                                  void* ws, size_t ws_bytes, void* stream, const int64_t* index = nullptr, int64_t rows = 0,
                                  const iisan_bert_dropout* drop = nullptr) {
    hipStream_t s = (hipStream_t)stream;
    if (drop) {
        IISAN_CHECK_SHAPE(drop->hidden_p >= 0.f && drop->hidden_p < 1.f, "bert dropout: hidden_p %.3f out of range", drop->hidden_p);
        IISAN_CHECK_SHAPE(drop->attn_p >= 0.f && drop->attn_p < 1.f, "bert dropout: attn_p %.3f out of range", drop->attn_p);
    }
    const bool dropping = drop && (drop->hidden_p > 0.f || drop->attn_p > 0.f);
    // never a silent fall-back to eval mode: the row kernels have train-mode instantiations for the mixed stream only
    IISAN_CHECK_SHAPE(!(dropping && g_resid32), "bert dropout: no train-mode instantiation for the fp32 residual stream of the dev switch resid32 = 1");
    // ... and for 768-wide rows only (rowops.hip): tap caches of the wide and the narrow towers are built in eval mode
    IISAN_CHECK_SHAPE(!(dropping && w->hidden != 768), "bert dropout: no train-mode instantiation at this width, hidden size %d runs in eval mode only "
                      "(drop == NULL or both probabilities 0)", w->hidden);
    // a DeBERTa struct (rel_emb != NULL): eval only — there is no train-mode instantiation of its embedding step or of its attention
    const bool deb = bert_is_deberta(w);
    IISAN_CHECK_SHAPE(!(dropping && deb), "deberta: the tower runs in eval mode only (drop == NULL or both probabilities 0): no train-mode "
                      "instantiation of the disentangled attention");
    IISAN_CHECK_SHAPE(M > 0, "bert_forward_taps: M must be positive");
    IISAN_TRY(check_common(false, w->hidden, w->layers, w->heads, w->mlp, n_taps, tap_layers));
    if (deb) {
        IISAN_TRY(deberta_check_struct(w));
        IISAN_CHECK_SHAPE(words >= 1, "deberta: %d words unsupported", words);
        IISAN_TRY(deberta_check_words(words, w->span));
    } else IISAN_TRY(bert_check_words(words, w->max_pos));
    // ... and the train-mode attention kernel keeps a whole head in LDS (bert_drop.hip): refused here, before any launch, never a silent fall-back
    IISAN_CHECK_SHAPE(!(dropping && words > 224), "bert dropout: no train-mode attention kernel past 224 words, titles of %d words run in eval mode only "
                      "(drop == NULL or both probabilities 0)", words);
    const int D = w->hidden, T = words;
    const Chunks c(M, chunk_items);
    WsCarver cv(ws, ws_bytes);
    EncBufs b;
    void *rel_own, *rel_ws;
    bert_carve(cv, b, w, c.Mc, T, &rel_own, &rel_ws);
    if (cv.overflow || !ws) {
        iisan_set_error("bert_forward_taps: workspace too small (%zu < %zu)", ws_bytes, cv.off);
        return IISAN_EWORKSPACE;
    }
    Products p{w->dtype16, D, w->mlp, T, w->heads, 0};
    const BertPlan plan = bert_plan(p, c);
    const bool full_blocks = g_full_blocks || w->full_blocks;
    const int live = full_blocks ? w->layers : max_tap(tap_layers, n_taps);     // see the ViT executor
    // DeBERTa without the caller's projected tables: the call projects those of its live layers into its workspace, once, before the chunks
    if (deb && !w->rel_proj && live > 0) IISAN_TRY(deberta_rel_project(w, live, rel_own, rel_ws, s));
    const void* rel = deb ? (w->rel_proj ? w->rel_proj : rel_own) : nullptr;
    for (int64_t m0 = 0; m0 < M; m0 += c.Mc) {
        const int64_t mc = (M - m0 < c.Mc) ? M - m0 : c.Mc;
        const BertChunk ch{{p, b, s, w->eps, plan.mixed, m0, mc, mc * T, taps + m0 * n_taps * D, n_taps}, w, plan.alias, dropping,
                           dropping ? drop->hidden_p : 0.f, dropping ? drop->attn_p : 0.f, dropping ? drop->seed : 0,
                           deb ? IISAN_TOWER_DEBERTA : IISAN_TOWER_BERT, rel};
        IISAN_TRY(ch.embed(text, index, rows));
        int k = tap_index(tap_layers, n_taps, 0);
        if (k >= 0) IISAN_TRY(ch.tap(k));
        for (int l = 0; l < live; ++l) {
            k = tap_index(tap_layers, n_taps, l + 1);
            if (l + 1 == live && !full_blocks) IISAN_TRY(ch.cls_block(l, k));
            else {
                IISAN_TRY(ch.full_block(l));
                if (k >= 0) IISAN_TRY(ch.tap(k));
            }
        }
    }
    return IISAN_OK;
}

extern "C" int iisan_bert_forward_taps(const iisan_bert_weights* w, const int64_t* text, int64_t M, int32_t words,
                                       const int32_t* tap_layers, int32_t n_taps, float* taps, int64_t chunk_items,
                                       void* ws, size_t ws_bytes, void* stream) {
    return bert_forward_taps_impl(w, text, M, words, tap_layers, n_taps, taps, chunk_items, ws, ws_bytes, stream);
}

extern "C" int iisan_bert_forward_taps_indexed(const iisan_bert_weights* w, const int64_t* table, int64_t rows,
                                               const int64_t* index, int64_t M, int32_t words, const int32_t* tap_layers,
                                               int32_t n_taps, float* taps, int64_t chunk_items, void* ws, size_t ws_bytes,
                                               void* stream) {
    IISAN_CHECK_SHAPE(rows > 0, "bert indexed: the table needs at least one row (rows = %lld)", (long long)rows);
    IISAN_CHECK_SHAPE(table != nullptr && index != nullptr, "bert indexed: null %s", table ? "index" : "table");
    IISAN_CHECK_SHAPE(M > 0, "bert indexed: M must be positive");
    return bert_forward_taps_impl(w, table, M, words, tap_layers, n_taps, taps, chunk_items, ws, ws_bytes, stream, index, rows);
}

extern "C" int iisan_bert_forward_taps_dropout(const iisan_bert_weights* w, const int64_t* text_or_table, int64_t rows,
                                               const int64_t* index, int64_t M, int32_t words, const int32_t* tap_layers,
                                               int32_t n_taps, float* taps, int64_t chunk_items, const iisan_bert_dropout* drop,
                                               void* ws, size_t ws_bytes, void* stream) {
    IISAN_CHECK_SHAPE(text_or_table != nullptr, "bert dropout: null text");
    IISAN_CHECK_SHAPE(!index || rows > 0, "bert dropout, indexed: the table needs at least one row (rows = %lld)", (long long)rows);
    IISAN_CHECK_SHAPE(M > 0, "bert dropout: M must be positive");
    return bert_forward_taps_impl(w, text_or_table, M, words, tap_layers, n_taps, taps, chunk_items, ws, ws_bytes, stream, index,
                                  index ? rows : 0, drop);
}

// The decisions vit_forward_taps_impl / bert_forward_taps_impl take before their first launch, for the towers' own shapes and no weights: the
// refusals that depend on these inputs, then vit_plan / bert_plan themselves.  `layers` is the shortest tower that has the tap.
extern "C" int32_t iisan_encoder_plan(int32_t tower, int32_t dtype16, int32_t hidden, int32_t heads, int32_t mlp, int32_t tokens, int64_t M,
                                      int64_t chunk_items, int32_t deepest_tap, int32_t full_blocks, int32_t folded) {
    IISAN_CHECK_SHAPE(tower == IISAN_TOWER_VIT || tower == IISAN_TOWER_BERT || tower == IISAN_TOWER_CLIP || tower == IISAN_TOWER_DEBERTA,
                      "encoder_plan: tower %d is neither ViT (0) nor BERT (1) nor CLIP (2) nor DeBERTa (3)", tower);
    const bool clip = tower == IISAN_TOWER_CLIP;
    IISAN_CHECK_SHAPE(M > 0, "encoder_plan: M must be positive");
    const int layers = deepest_tap > 1 ? deepest_tap : 1;
    if (tower == IISAN_TOWER_DEBERTA) {     // the BERT executor's plan behind the DeBERTa refusals; `folded` carries the span
        IISAN_TRY(check_common(false, hidden, layers, heads, mlp, 1, &deepest_tap));
        IISAN_TRY(deberta_check_span(folded));
        IISAN_CHECK_SHAPE(tokens >= 1, "deberta: %d words unsupported", tokens);
        IISAN_TRY(deberta_check_words(tokens, folded));
        tower = IISAN_TOWER_BERT;
    }
    IISAN_TRY(check_common(tower != IISAN_TOWER_BERT, hidden, layers, heads, mlp, 1, &deepest_tap));
    IISAN_TRY(tower != IISAN_TOWER_BERT ? vit_check_tokens(tokens) : bert_check_words(tokens, tokens));
    const bool full = g_full_blocks || full_blocks;
    const Chunks c(M, chunk_items);
    Products p{dtype16, hidden, mlp, tokens, heads, clip ? 1 : 0};
    if (tower == IISAN_TOWER_BERT) {
        const BertPlan plan = bert_plan(p, c);
        return (plan.mixed ? 1 : 0) | (plan.alias ? 2 : 0) | (p.f1blk ? 4 : 0);
    }
    const VitPlan plan = vit_plan(p, full ? layers : deepest_tap, full || p.hd80(), folded != 0, c, clip);
    return (int32_t)plan.st | (p.f1blk ? 4 : 0) | (p.xblk ? 8 : 0) | (plan.folds ? 16 : 0) | (p.hd80() ? 32 : 0);
}
