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
    void* QKV;      // [Tp, 3D] 16-bit
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

Gemm16Args gemm_args(int mode, const void* A, int K, const void* W, const float* bias, void* out, int N, int64_t M, int qkv_S = 0,
                     int qkv_heads = 0, int qkv_which0 = 0, const float* rowstat = nullptr) {
    Gemm16Args a{};
    a.A = A; a.W = W; a.bias = bias; a.out = out;
    a.M = M; a.N = N; a.K = K; a.lda = K; a.ldw = K; a.ldo = N;
    a.qkv_S = qkv_S; a.qkv_heads = qkv_heads; a.qkv_which0 = qkv_which0;
    a.rowstat = rowstat;
    return a;
}

// F1 block-major?  Decided once per call: only when BOTH products — FC1 (GELU, `rowstat`: LayerNorm in its epilogue) and FC2 (`fc2_mode`:
// EPI_OUT16 or EPI_STREAM16) — run on gemm16_h256 with the flag for every chunk size of the call (the last chunk may be shorter)
bool f1_blk32(int dt, int D, int F, int64_t M, int64_t Mc, int T, const float* rowstat, int fc2_mode, float* rowpart) {
    if (g_blk32 < 1) return false;
    for (int64_t mc : {Mc, M % Mc == 0 ? Mc : M % Mc}) {
        const int64_t tok = mc * T;
        Gemm16Args f1 = gemm_args(EPI_GELU16, nullptr, D, nullptr, nullptr, nullptr, F, tok, 0, 0, 0, rowstat);
        Gemm16Args f2 = gemm_args(fc2_mode, nullptr, F, nullptr, nullptr, nullptr, D, tok, fc2_mode == EPI_STREAM16 ? T : 0);
        f1.out_blk32 = 1;
        f2.a_blk32 = 1; f2.rowpart = rowpart;
        if (gemm16_route(dt, EPI_GELU16, f1) != G16_H256 || gemm16_route(dt, fc2_mode, f2) != G16_H256) return false;
    }
    return true;
}

// The ViT stream block-major?  Only on the product route (VS_STREAM) with F1 block-major, and only when every product that touches the
// stream takes the flags for every chunk size of the call: QKV and FC1 (A), O and FC2 (read-modify-write), the K/V product of a CLS-only
// last block (A)
bool x16_blk32(int dt, int D, int F, int heads, int64_t M, int64_t Mc, int T, bool full_blocks, const float* rowstat, float* rowpart) {
    if (g_blk32 < 2) return false;
    for (int64_t mc : {Mc, M % Mc == 0 ? Mc : M % Mc}) {
        const int64_t tok = mc * T;
        Gemm16Args q = gemm_args(EPI_QKVH16, nullptr, D, nullptr, nullptr, nullptr, 3 * D, tok, T, heads, 0, rowstat);
        Gemm16Args kv = gemm_args(EPI_QKVH16, nullptr, D, nullptr, nullptr, nullptr, 2 * D, tok, T, heads, 1, rowstat);
        Gemm16Args f1 = gemm_args(EPI_GELU16, nullptr, D, nullptr, nullptr, nullptr, F, tok, 0, 0, 0, rowstat);
        Gemm16Args o = gemm_args(EPI_STREAM16, nullptr, D, nullptr, nullptr, nullptr, D, tok, T), f2 = gemm_args(EPI_STREAM16, nullptr, F, nullptr, nullptr, nullptr, D, tok, T);
        q.a_blk32 = kv.a_blk32 = f1.a_blk32 = f1.out_blk32 = o.out_blk32 = f2.a_blk32 = f2.out_blk32 = 1;
        o.rowpart = f2.rowpart = rowpart;
        auto h256 = [&](int mode, const Gemm16Args& a) { return gemm16_route(dt, mode, a) == G16_H256; };
        if (!(h256(EPI_QKVH16, q) && h256(EPI_GELU16, f1) && h256(EPI_STREAM16, o) && h256(EPI_STREAM16, f2) && (full_blocks || h256(EPI_QKVH16, kv))))
            return false;
    }
    return true;
}

// the FC1 -> FC2 pair of an all-token block: F1 = GELU(A W1^T + b1) (rowstat: LayerNorm in the epilogue), out = F1 W2^T + b2
int gemm_fc1(int dt, const void* A, int D, const void* W, const float* bias, const float* rowstat, void* F1, int F, int64_t M, bool f1blk, hipStream_t s,
             bool a_blk = false) {
    Gemm16Args a = gemm_args(EPI_GELU16, A, D, W, bias, F1, F, M, 0, 0, 0, rowstat);
    a.out_blk32 = f1blk; a.a_blk32 = a_blk;
    return launch_gemm16(dt, EPI_GELU16, a, s);
}
int gemm_fc2(int dt, const void* F1, int F, const void* W, const float* bias, void* out, int D, int64_t M, bool f1blk, hipStream_t s) {
    Gemm16Args a = gemm_args(EPI_OUT16, F1, F, W, bias, out, D, M);
    a.a_blk32 = f1blk;
    return launch_gemm16(dt, EPI_OUT16, a, s);
}

int gemm(int dt, int mode, const void* A, int K, const void* W, const float* bias, void* out, int N, const float* resid,
         int64_t M, hipStream_t s, const float* pos = nullptr, int patch_P = 0, int qkv_S = 0, int qkv_heads = 0,
         int qkv_which0 = 0) {
    Gemm16Args a = gemm_args(mode, A, K, W, bias, out, N, M, qkv_S, qkv_heads, qkv_which0);
    a.resid = resid; a.pos = pos; a.patch_P = patch_P;
    return launch_gemm16(dt, mode, a, s);
}

// LN(x) W^T + b with the LayerNorm in the epilogue: A = the stream, W / bias = the folded set, rowstat = the rows' rstd
int gemm_ln(int dt, int mode, const void* X16, int K, const void* Wf, const float* bf, const float* rs, void* out, int N,
            int64_t M, hipStream_t s, int qkv_S = 0, int qkv_heads = 0, int qkv_which0 = 0, bool x_blk = false) {
    Gemm16Args a = gemm_args(mode, X16, K, Wf, bf, out, N, M, qkv_S, qkv_heads, qkv_which0, rs);
    a.a_blk32 = x_blk;       // the stream is block-major
    return launch_gemm16(dt, mode, a, s);
}

// Last live block: K and V for every token (head-major; the q third of the buffer is left untouched), Q for the CLS rows
// only.  Hc (in) / Qc (out) are compact [mc, D] 16-bit views: Hc = the CLS rows of the block's 16-bit input H.
int kv_all_q_cls(int dt, const iisan_layer_weights& L, const void* H, void* QKV, const void* Hc, void* Qc, int64_t tok,
                 int64_t mc, int T, int heads, int D, hipStream_t s) {
    const size_t e16 = 2;
    IISAN_TRY(gemm(dt, EPI_QKVH16, H, D, (const char*)L.qkv_w + (size_t)D * D * e16, L.qkv_b + D, QKV, 2 * D, nullptr, tok, s,
                   nullptr, 0, T, heads, 1));
    IISAN_TRY(gemm(dt, EPI_OUT16, Hc, D, L.qkv_w, L.qkv_b, Qc, D, nullptr, mc, s));
    return IISAN_OK;
}

int tap_index(const int32_t* tap_layers, int n, int layer) {
    for (int k = 0; k < n; ++k)
        if (tap_layers[k] == layer) return k;
    return -1;
}

// process-wide OVERRIDE of the weights structs' `full_blocks` field (bench.py, tests; not declared in include/iisan_hip.h):
// 1 = run every block of the tower on every token, as the reference does
int g_full_blocks = 0;

int max_tap(const int32_t* tap_layers, int n) {
    int m = 0;
    for (int k = 0; k < n; ++k) m = tap_layers[k] > m ? tap_layers[k] : m;
    return m;
}

int check_common(int hidden, int layers, int heads, int mlp, int n_taps, const int32_t* tap_layers) {
    // the widths the row kernels are instantiated at (rowops.hip): ViT-B / BERT-base, ViT-L / BERT-large, and the narrow towers — BERT-tiny
    // (128), ViT-tiny (192), BERT-mini (256), ViT-small (384)
    IISAN_CHECK_SHAPE(hidden == 768 || hidden == 1024 || hidden == 128 || hidden == 192 || hidden == 256 || hidden == 384,
                      "encoder hidden size %d not supported: the supported widths are 768 (12 heads) and 1024 (16 heads), "
                      "and 128, 192, 256, 384 (2, 3, 4, 6 heads)", hidden);
    IISAN_CHECK_SHAPE(heads > 0 && hidden == heads * 64, "encoder head_dim must be 64 (hidden %d, heads %d; supported: 768 / 12 and 1024 / 16, "
                      "128 / 2, 192 / 3, 256 / 4, 384 / 6)", hidden, heads);
    IISAN_CHECK_SHAPE(layers >= 1 && layers <= IISAN_MAX_LAYERS, "encoder layers %d out of range", layers);
    IISAN_CHECK_SHAPE(mlp % 128 == 0, "encoder mlp size %d must be a multiple of 128", mlp);
    IISAN_CHECK_SHAPE(n_taps >= 1 && tap_layers, "need at least one tap layer");
    for (int k = 0; k < n_taps; ++k)
        IISAN_CHECK_SHAPE(tap_layers[k] >= 0 && tap_layers[k] <= layers, "tap layer %d outside 0..%d", tap_layers[k], layers);
    return IISAN_OK;
}

}  // namespace

IISAN_DEV_KNOB(full_blocks, g_full_blocks);
IISAN_DEV_KNOB(resid32, g_resid32);
IISAN_DEV_KNOB(ln_fold, g_ln_fold);
IISAN_DEV_KNOB(blk32, g_blk32);
// (the LayerNorm-folded routes — fold_ln_weights, the stream statistics, the block-major stream — are 768 wide: a 1024-wide tower and the
//  narrow ones (128 - 384) run on the LayerNorm-image route whatever ln_fold says, and ask for no folded set)
static int vit_fold_layers(const iisan_vit_weights* w) {
    return (!g_resid32 && g_ln_fold && w->dtype16 == IISAN_F16 && w->hidden == 768) ? w->layers : 0;
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
    if (w->dtype16 != IISAN_F16 || w->hidden != 768) return 0;
    return (size_t)w->layers * (vit_fold_w_elems(w) * 2 + (size_t)(3 * w->hidden + w->mlp) * 4);
}

extern "C" int iisan_vit_fold_layernorm(const iisan_vit_weights* w, void* folded, size_t bytes, void* stream) {
    const size_t need = iisan_vit_fold_bytes(w);
    IISAN_CHECK_SHAPE(need > 0, "vit_fold_layernorm: fp16 operands and hidden size 768 only");
    if (!folded || bytes < need) {
        iisan_set_error("vit_fold_layernorm: buffer too small (%zu < %zu)", bytes, need);
        return IISAN_EWORKSPACE;
    }
    IISAN_CHECK_SHAPE(w->layers >= 1 && w->layers <= IISAN_MAX_LAYERS, "vit_fold_layernorm: layers %d out of range", w->layers);
    return vit_fold_all(w, w->layers, true, (char*)folded, (float*)((char*)folded + (size_t)w->layers * vit_fold_w_elems(w) * 2), (hipStream_t)stream);
}

extern "C" size_t iisan_vit_forward_taps_ws_bytes(const iisan_vit_weights* w, int64_t M, int64_t chunk_items) {
    const int64_t Mc = (chunk_items > 0 && chunk_items < M) ? chunk_items : M;
    const int P = (w->image / w->patch) * (w->image / w->patch);
    const int pd = w->channels * w->patch * w->patch;
    WsCarver c(nullptr, 0);
    EncBufs b;
    return carve(c, b, Mc * (P + 1), Mc, w->hidden, w->mlp > pd ? w->mlp : pd, 0, vit_fold_layers(w), w->folded == nullptr);
}

namespace {

// How one call carries the residual stream of the pre-LN tower; decided once per call (vit_strategy).  Each strategy is three steps of
// VitChunk, every one a complete launch list: `open` (the stream becomes hidden state l; LN1), a full block, `close` (the last hidden
// state, when it is tapped).
enum VitStrategy {
    VS_RESID32,     // dev knob resid32: the whole stream fp32 in X, LayerNorm images in H
    VS_IMAGE,       // mixed stream (fp16 rows in X16, fp32 CLS rows in Xc), LayerNorm images in H: ln_fold = 0, bf16 operands, small batches
    VS_FOLD,        // mixed stream, no image: the add kernels leave rstd per row, the QKV / FC1 products apply LayerNorm (ln_fold = 1)
    VS_STREAM,      // ... and no add kernels: the O / FC2 products add into the stream in their epilogues (ln_fold = 2, the product route)
};

// LayerNorm in the epilogues of the QKV / FC1 products (g_ln_fold) only where those products run on the kernel that has it, and the
// residual adds in the epilogues of the O / FC2 products likewise — for every chunk size of this call (the last chunk may be shorter)
VitStrategy vit_strategy(const iisan_vit_weights* w, const EncBufs& b, int live, bool full_blocks, int64_t M, int64_t Mc, int T) {
    if (g_resid32) return VS_RESID32;
    if (!b.Wf || live == 0 || w->hidden != 768) return VS_IMAGE;       // (any other width: b.Wf is null already — vit_fold_layers)
    const int dt = w->dtype16, D = w->hidden, F = w->mlp;
    bool fold = true, stream = g_ln_fold >= 2;
    for (int64_t mc : {Mc, M % Mc == 0 ? Mc : M % Mc}) {
        const int64_t tok = mc * T;
        auto h256 = [&](int mode, const Gemm16Args& a) { return gemm16_route(dt, mode, a) == G16_H256; };
        fold = fold && h256(EPI_QKVH16, gemm_args(EPI_QKVH16, nullptr, D, nullptr, nullptr, nullptr, 3 * D, tok, T, w->heads, 0, b.RS)) &&
               h256(EPI_GELU16, gemm_args(EPI_GELU16, nullptr, D, nullptr, nullptr, nullptr, F, tok, 0, 0, 0, b.RS)) &&
               (full_blocks || h256(EPI_QKVH16, gemm_args(EPI_QKVH16, nullptr, D, nullptr, nullptr, nullptr, 2 * D, tok, T, w->heads, 1, b.RS)));
        Gemm16Args o = gemm_args(EPI_STREAM16, nullptr, D, nullptr, nullptr, nullptr, D, tok, T), f = gemm_args(EPI_STREAM16, nullptr, F, nullptr, nullptr, nullptr, D, tok, T);
        o.rowpart = f.rowpart = b.RP;
        stream = stream && h256(EPI_STREAM16, o) && h256(EPI_STREAM16, f);
    }
    return !fold ? VS_IMAGE : stream ? VS_STREAM : VS_FOLD;
}

constexpr int MX_ADD_STAT = MX_D1 | MX_RESV | MX_STAT;       // x += d (fp16 stream, fp32 CLS rows); row statistics

// One chunk of a ViT forward: mc items, tok = mc * T token rows, tp = their rows of the tap tensor.
// The O / FC2 products of resid32 / image / fold emit 16-bit DELTAS (dO in D16, dF in D16b); the residual add is fused into a later
// LayerNorm kernel (HBM-bound) instead of a read-modify-write GEMM epilogue.  Pre-LN tower, resid32 / image: LN2 computes LN(x + dO)
// WITHOUT writing x back; the next open step adds both deltas, (x + dO) + dF in fp32 — the same value — and writes x once per block
// instead of twice.
struct VitChunk {
    const iisan_vit_weights* w; const EncBufs& b; VitStrategy st; hipStream_t s;
    int dt, D, F, T, heads; float eps;
    int64_t mc, tok; float* tp; int n_taps;
    bool f1blk;     // F1 of the full blocks is block-major (f1_blk32, decided once per call)
    bool xblk;      // ... and so is the stream X16 (x16_blk32; VS_STREAM only)

    bool mixed() const { return st != VS_RESID32; }
    const iisan_layer_weights& layer(int l) const { return w->layer[l]; }
    // the folded set of layer l (vit_fold_all)
    char* Wf_qkv(int l) const { return (char*)b.Wf + (size_t)l * (3 * D + F) * D * 2; }
    char* Wf_fc1(int l) const { return Wf_qkv(l) + (size_t)3 * D * D * 2; }
    float* bf_qkv(int l) const { return b.Bf + (size_t)l * (3 * D + F); }
    float* bf_fc1(int l) const { return bf_qkv(l) + 3 * D; }

    // index != null: `img` is a resident uint8 catalogue of `rows` images and item m of the chunk is its row index[m]
    int embed(const void* img, int img_u8, const int64_t* index = nullptr, int64_t rows = 0) const {
        const int P = T - 1, pd = w->channels * w->patch * w->patch;
        if (index) IISAN_TRY(launch_vit_im2col_indexed(dt, (const uint8_t*)img, rows, index, b.F1, mc, w->channels, w->image, w->patch, s));
        else IISAN_TRY(launch_vit_im2col(dt, img, img_u8, b.F1, mc, w->channels, w->image, w->patch, s));
        // patch embedding: resid32 = fp32 token rows with the position embedding added (128x128 kernel); mixed = 16-bit rows on the
        // production GEMM (gemm16_h256, 0.40 against 0.59 ms at bs = 128), the position table is added by block 0's open step
        if (mixed()) IISAN_TRY(gemm(dt, EPI_PATCH16, b.F1, pd, w->patch_w, w->patch_b, b.D16b, D, nullptr, mc * P, s, nullptr, P));
        else IISAN_TRY(gemm(dt, EPI_PATCH32, b.F1, pd, w->patch_w, w->patch_b, b.X, D, nullptr, mc * P, s, w->pos_emb, P));
        // CLS rows: cls + pos[0] — into the fp32 stream (token-major) or into the compact fp32 CLS stream
        return launch_vit_cls_rows(mixed() ? b.Xc : b.X, w->cls_token, w->pos_emb, mc, mixed() ? 1 : T, D, s);
    }
    // the tapped rows of the current hidden state: CLS rows of X (stride T) or the compact CLS stream itself
    int tap(int k) const { return mixed() ? launch_gather_cls(b.Xc, tp, mc, 1, D, n_taps, k, s) : launch_gather_cls(b.X, tp, mc, T, D, n_taps, k, s); }

    // ---- VS_RESID32 ------------------------------------------------------------------------------------------------------------
    int open_resid32(int l) const {     // x += dO + dF of block l - 1 ; h = LN1(x)
        const iisan_layer_weights& L = layer(l);
        if (l == 0) return launch_add2_layernorm768(dt, b.X, nullptr, nullptr, L.ln1_w, L.ln1_b, eps, nullptr, b.H, nullptr, tok, D, s);
        return launch_add2_layernorm768(dt, b.X, b.D16, b.D16b, L.ln1_w, L.ln1_b, eps, b.X, b.H, nullptr, tok, D, s);
    }
    int full_resid32(int l) const {
        const iisan_layer_weights& L = layer(l);
        IISAN_TRY(gemm(dt, EPI_QKVH16, b.H, D, L.qkv_w, L.qkv_b, b.QKV, 3 * D, nullptr, tok, s, nullptr, 0, T, heads));
        IISAN_TRY(launch_attention16(dt, b.QKV, nullptr, b.H, mc, T, heads, s));
        IISAN_TRY(gemm(dt, EPI_OUT16, b.H, D, L.o_w, L.o_b, b.D16, D, nullptr, tok, s));
        // h = LN2(x + dO)   (x itself is updated by the next open step)
        IISAN_TRY(launch_add_layernorm768(dt, b.X, b.D16, L.ln2_w, L.ln2_b, eps, nullptr, b.H, nullptr, tok, D, s));
        IISAN_TRY(gemm(dt, EPI_GELU16, b.H, D, L.fc1_w, L.fc1_b, b.F1, F, nullptr, tok, s));
        return gemm(dt, EPI_OUT16, b.F1, F, L.fc2_w, L.fc2_b, b.D16b, D, nullptr, tok, s);
    }
    int close_resid32() const { return launch_add2_layernorm768(dt, b.X, b.D16, b.D16b, nullptr, nullptr, eps, b.X, nullptr, nullptr, tok, D, s); }

    // ---- VS_IMAGE ----------------------------------------------------------------------------------------------------------------
    int open_image(int l) const {
        const iisan_layer_weights& L = layer(l);
        if (l == 0)     // position table + 16-bit patch embedding -> fp16 stream of the patch rows (the CLS rows are in Xc already) + LN image
            return launch_layernorm768_mixed(dt, MX_SRC32 | MX_POSROW | MX_D1 | MX_RESV | MX_LN, w->pos_emb, b.X16, b.Xc, b.D16b, nullptr, L.ln1_w, L.ln1_b, eps, b.H, mc, T, D, s);
        return launch_layernorm768_mixed(dt, MX_D1 | MX_D2 | MX_RESV | MX_LN, nullptr, b.X16, b.Xc, b.D16, b.D16b, L.ln1_w, L.ln1_b, eps, b.H, mc, T, D, s);
    }
    int full_image(int l) const {
        const iisan_layer_weights& L = layer(l);
        IISAN_TRY(gemm(dt, EPI_QKVH16, b.H, D, L.qkv_w, L.qkv_b, b.QKV, 3 * D, nullptr, tok, s, nullptr, 0, T, heads));
        IISAN_TRY(launch_attention16(dt, b.QKV, nullptr, b.H, mc, T, heads, s));
        IISAN_TRY(gemm(dt, EPI_OUT16, b.H, D, L.o_w, L.o_b, b.D16, D, nullptr, tok, s));
        // h = LN2(x + dO)   (x itself is updated by the next open step)
        IISAN_TRY(launch_layernorm768_mixed(dt, MX_D1 | MX_LN, nullptr, b.X16, b.Xc, b.D16, nullptr, L.ln2_w, L.ln2_b, eps, b.H, mc, T, D, s));
        IISAN_TRY(gemm_fc1(dt, b.H, D, L.fc1_w, L.fc1_b, nullptr, b.F1, F, tok, f1blk, s));
        return gemm_fc2(dt, b.F1, F, L.fc2_w, L.fc2_b, b.D16b, D, tok, f1blk, s);
    }
    // only the CLS rows of the last hidden state are consumed
    int close_image() const { return launch_layernorm768_mixed(dt, MX_D1 | MX_D2 | MX_RESV | MX_CLSONLY, nullptr, b.X16, b.Xc, b.D16, b.D16b, nullptr, nullptr, eps, nullptr, mc, T, D, s); }

    // ---- VS_FOLD: the stream + rstd per row; LN1 / LN2 are applied by the epilogues of the QKV / FC1 products -------------------------
    int patches_to_stream() const {     // position table + 16-bit patch embedding -> fp16 stream of the patch rows (the CLS rows are in Xc already)
        return launch_layernorm768_mixed(dt, MX_SRC32 | MX_POSROW | MX_ADD_STAT | (xblk ? MX_BLK32 : 0), w->pos_emb, b.X16, b.Xc, b.D16b, nullptr, nullptr, nullptr, eps, nullptr, mc, T, D, s, b.RS);
    }
    int open_fold(int l) const {
        if (l == 0) return patches_to_stream();
        // x += dF of block l - 1 (x + dO is in the stream already: that block wrote it in its LN2 step)
        return launch_layernorm768_mixed(dt, MX_ADD_STAT, nullptr, b.X16, b.Xc, b.D16b, nullptr, nullptr, nullptr, eps, nullptr, mc, T, D, s, b.RS);
    }
    int full_fold(int l) const {
        const iisan_layer_weights& L = layer(l);
        IISAN_TRY(gemm_ln(dt, EPI_QKVH16, b.X16, D, Wf_qkv(l), bf_qkv(l), b.RS, b.QKV, 3 * D, tok, s, T, heads));
        IISAN_TRY(launch_attention16(dt, b.QKV, nullptr, b.H, mc, T, heads, s));
        IISAN_TRY(gemm(dt, EPI_OUT16, b.H, D, L.o_w, L.o_b, b.D16, D, nullptr, tok, s));
        // x += dO (written: the FC1 product reads the stream); LN2 in the FC1 product's epilogue
        IISAN_TRY(launch_layernorm768_mixed(dt, MX_ADD_STAT, nullptr, b.X16, b.Xc, b.D16, nullptr, nullptr, nullptr, eps, nullptr, mc, T, D, s, b.RS));
        IISAN_TRY(gemm_fc1(dt, b.X16, D, Wf_fc1(l), bf_fc1(l), b.RS, b.F1, F, tok, f1blk, s));
        return gemm_fc2(dt, b.F1, F, L.fc2_w, L.fc2_b, b.D16b, D, tok, f1blk, s);
    }
    // x + dO is in the stream: the CLS rows take dF
    int close_fold() const { return launch_layernorm768_mixed(dt, MX_D1 | MX_RESV | MX_CLSONLY, nullptr, b.X16, b.Xc, b.D16b, nullptr, nullptr, nullptr, eps, nullptr, mc, T, D, s); }

    // ---- VS_STREAM: ... and the O / FC2 products add into the stream and leave its row statistics --------------------------------------
    // x += A W^T + bias in the stream (fp16 rows in place, the CLS rows' fp32 stream through the finalize step); rstd of the new rows
    int gemm_stream(const void* A, int K, const void* W, const float* bias, bool a_blk = false) const {
        Gemm16Args a = gemm_args(EPI_STREAM16, A, K, W, bias, b.X16, D, tok, T);
        a.rowpart = b.RP; a.a_blk32 = a_blk; a.out_blk32 = xblk;
        IISAN_TRY(launch_gemm16(dt, EPI_STREAM16, a, s));
        return launch_stream_stats_finalize(b.RP, D / 64, ceil_div(tok, 256) * 256, b.X16, b.Xc, b.RS, eps, mc, T, s, xblk);
    }
    int open_stream(int l) const {
        if (l == 0) return patches_to_stream();
        return IISAN_OK;        // the FC2 product of block l - 1 added into the stream and left its statistics
    }
    int full_stream(int l) const {
        const iisan_layer_weights& L = layer(l);
        IISAN_TRY(gemm_ln(dt, EPI_QKVH16, b.X16, D, Wf_qkv(l), bf_qkv(l), b.RS, b.QKV, 3 * D, tok, s, T, heads, 0, xblk));
        IISAN_TRY(launch_attention16(dt, b.QKV, nullptr, b.H, mc, T, heads, s));
        IISAN_TRY(gemm_stream(b.H, D, L.o_w, L.o_b));
        IISAN_TRY(gemm_fc1(dt, b.X16, D, Wf_fc1(l), bf_fc1(l), b.RS, b.F1, F, tok, f1blk, s, xblk));
        return gemm_stream(b.F1, F, L.fc2_w, L.fc2_b, f1blk);
    }
    int close_stream() const { return IISAN_OK; }       // the stream is the last hidden state already

    // ---- the last LIVE block when later blocks are dead code: only the CLS token's output is consumed.  K/V are computed for every token,
    // but attention, O, LN2, FC1, FC2 and the closing residual add run on one row per item; its output goes to tap k
    int cls_block(int l, int k) const {
        const iisan_layer_weights& L = layer(l);
        // CLS rows only: compact [mc, D] 16-bit views in their own scratch
        void* Hc = b.Cls;
        void* Qc = (char*)b.Cls + (size_t)b.Mcp * D * 2;
        if (st == VS_FOLD || st == VS_STREAM) {
            // K / V of every token from the stream (LN1 in the epilogue); the CLS rows' LN1 image from their fp32 stream
            IISAN_TRY(launch_layernorm768(dt, b.Xc, L.ln1_w, L.ln1_b, eps, Hc, nullptr, mc, D, s));
            IISAN_TRY(gemm_ln(dt, EPI_QKVH16, b.X16, D, Wf_qkv(l) + (size_t)D * D * 2, bf_qkv(l) + D, b.RS, b.QKV, 2 * D, tok, s, T, heads, 1, xblk));
            IISAN_TRY(gemm(dt, EPI_OUT16, Hc, D, L.qkv_w, L.qkv_b, Qc, D, nullptr, mc, s));
        } else {
            IISAN_TRY(launch_gather_rows16(b.H, Hc, mc, T, D, s));            // CLS rows of LN1(x)
            IISAN_TRY(kv_all_q_cls(dt, L, b.H, b.QKV, Hc, Qc, tok, mc, T, heads, D, s));
        }
        IISAN_TRY(launch_attention_cls16(dt, b.QKV, nullptr, b.H, mc, T, heads, s, Qc));
        float* Xc = (float*)b.QKV;      // free once the CLS attention has run (stream order)
        IISAN_TRY(gemm(dt, EPI_OUT16, b.H, D, L.o_w, L.o_b, b.D16, D, nullptr, mc, s));
        if (mixed()) IISAN_TRY(launch_gather_cls(b.Xc, Xc, mc, 1, D, 1, 0, s)); else IISAN_TRY(launch_gather_cls(b.X, Xc, mc, T, D, 1, 0, s));
        IISAN_TRY(launch_add_layernorm768(dt, Xc, b.D16, L.ln2_w, L.ln2_b, eps, Xc, b.H, nullptr, mc, D, s));
        IISAN_TRY(gemm(dt, EPI_GELU16, b.H, D, L.fc1_w, L.fc1_b, b.F1, F, nullptr, mc, s));
        IISAN_TRY(gemm(dt, EPI_OUT16, b.F1, F, L.fc2_w, L.fc2_b, b.D16, D, nullptr, mc, s));
        IISAN_TRY(launch_add_layernorm768(dt, Xc, b.D16, nullptr, nullptr, eps, Xc, nullptr, nullptr, mc, D, s));
        return launch_gather_cls(Xc, tp, mc, 1, D, n_taps, k, s);     // hidden state `live` (before any final LayerNorm)
    }
};

// the three steps of every strategy, indexed by VitStrategy
const struct { int (VitChunk::*open)(int) const; int (VitChunk::*full)(int) const; int (VitChunk::*close)() const; } VIT_STEPS[] = {
    {&VitChunk::open_resid32, &VitChunk::full_resid32, &VitChunk::close_resid32},
    {&VitChunk::open_image, &VitChunk::full_image, &VitChunk::close_image},
    {&VitChunk::open_fold, &VitChunk::full_fold, &VitChunk::close_fold},
    {&VitChunk::open_stream, &VitChunk::full_stream, &VitChunk::close_stream},
};

}  // namespace

// index != null: `images` is a resident uint8 catalogue [rows, C, R, R] and slot m reads row index[m] (the chunk loop offsets the
// index, never the catalogue)
static int vit_forward_taps_impl(const iisan_vit_weights* w, const void* images, int img_u8, int64_t M,
                                 const int32_t* tap_layers, int32_t n_taps, float* taps, int64_t chunk_items,
                                 void* ws, size_t ws_bytes, void* stream, const int64_t* index = nullptr, int64_t rows = 0) {
    hipStream_t s = (hipStream_t)stream;
    IISAN_CHECK_SHAPE(M > 0, "vit_forward_taps: M must be positive");
    IISAN_TRY(check_common(w->hidden, w->layers, w->heads, w->mlp, n_taps, tap_layers));
    IISAN_CHECK_SHAPE(w->patch % 8 == 0 && w->image % w->patch == 0, "vit: patch %d / image %d unsupported", w->patch, w->image);
    const int D = w->hidden, F = w->mlp, P = (w->image / w->patch) * (w->image / w->patch), T = P + 1;
    const int pd = w->channels * w->patch * w->patch;
    IISAN_CHECK_SHAPE(pd % 64 == 0, "vit: patch vector length %d must be a multiple of 64", pd);
    // (past 224 tokens the attention steps run the streaming-softmax kernel, attn16_long.hip; everything else takes T as it comes)
    IISAN_CHECK_SHAPE(T <= 1024, "vit: %d tokens per image > 1024 not supported", T);
    const int64_t Mc = (chunk_items > 0 && chunk_items < M) ? chunk_items : M;
    WsCarver c(ws, ws_bytes);
    EncBufs b;
    carve(c, b, Mc * T, Mc, D, F > pd ? F : pd, 0, vit_fold_layers(w), w->folded == nullptr);
    if (w->folded && b.RS) {       // the caller folded once (iisan_vit_fold_layernorm)
        b.Wf = const_cast<void*>(w->folded);
        b.Bf = (float*)((char*)b.Wf + (size_t)w->layers * vit_fold_w_elems(w) * 2);
    }
    if (c.overflow || !ws) {
        iisan_set_error("vit_forward_taps: workspace too small (%zu < %zu)", ws_bytes, c.off);
        return IISAN_EWORKSPACE;
    }
    const bool full_blocks = g_full_blocks || w->full_blocks;
    // Blocks after the deepest tapped hidden state are dead code (Versa configurations tap a prefix of the tower)
    const int live = full_blocks ? w->layers : max_tap(tap_layers, n_taps);
    const VitStrategy st = vit_strategy(w, b, live, full_blocks, M, Mc, T);
    const auto& step = VIT_STEPS[st];
    const bool xblk = st == VS_STREAM && x16_blk32(w->dtype16, D, F, w->heads, M, Mc, T, full_blocks, b.RS, b.RP);
    const bool f1blk = xblk || (st != VS_RESID32 && f1_blk32(w->dtype16, D, F, M, Mc, T, st >= VS_FOLD ? b.RS : nullptr, st == VS_STREAM ? EPI_STREAM16 : EPI_OUT16, b.RP));
    if (st >= VS_FOLD && !w->folded) IISAN_TRY(vit_fold_all(w, live, full_blocks, (char*)b.Wf, b.Bf, s));
    const int64_t img_elems = (int64_t)w->channels * w->image * w->image;
    for (int64_t m0 = 0; m0 < M; m0 += Mc) {
        const int64_t mc = (M - m0 < Mc) ? M - m0 : Mc;
        const VitChunk ch{w, b, st, s, w->dtype16, D, F, T, w->heads, w->eps, mc, mc * T, taps + m0 * n_taps * D, n_taps, f1blk, xblk};
        if (index) IISAN_TRY(ch.embed(images, 1, index + m0, rows));
        else IISAN_TRY(ch.embed(img_u8 ? (const void*)((const uint8_t*)images + m0 * img_elems) : (const void*)((const float*)images + m0 * img_elems), img_u8));
        int k = tap_index(tap_layers, n_taps, 0);
        if (k >= 0) IISAN_TRY(ch.tap(k));
        for (int l = 0; l < live; ++l) {
            IISAN_TRY((ch.*step.open)(l));       // -> the stream is hidden state l
            k = tap_index(tap_layers, n_taps, l);
            if (k >= 0 && l > 0) IISAN_TRY(ch.tap(k));
            if (l + 1 < live || full_blocks) IISAN_TRY((ch.*step.full)(l));
            else IISAN_TRY(ch.cls_block(l, tap_index(tap_layers, n_taps, live)));
        }
        k = full_blocks ? tap_index(tap_layers, n_taps, w->layers) : -1;
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

extern "C" size_t iisan_bert_forward_taps_ws_bytes(const iisan_bert_weights* w, int64_t M, int32_t words, int64_t chunk_items) {
    const int64_t Mc = (chunk_items > 0 && chunk_items < M) ? chunk_items : M;
    WsCarver c(nullptr, 0);
    EncBufs b;
    return carve(c, b, Mc * words, Mc, w->hidden, w->mlp, Mc * words);
}

// index != null: `text` is a resident table [rows, 2W] and slot m reads row index[m] (the chunk loop offsets the index, never the table)
// drop: null or both probabilities 0 = eval mode, the launch sequence below unchanged; otherwise the attention kernel of bert_drop.hip takes
// the place of the eval-mode one, and the embedding and add + LayerNorm steps run their train-mode instantiations (a RowKeep instead of
// null; rowops.hip) — sites and indices: include/iisan_hip.h, iisan_bert_dropout
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
    const float hp = dropping ? drop->hidden_p : 0.f, ap = dropping ? drop->attn_p : 0.f;
    const uint64_t seed = dropping ? drop->seed : 0;
    IISAN_CHECK_SHAPE(M > 0, "bert_forward_taps: M must be positive");
    IISAN_TRY(check_common(w->hidden, w->layers, w->heads, w->mlp, n_taps, tap_layers));
    IISAN_CHECK_SHAPE(words >= 1 && words <= w->max_pos && words <= 1024, "bert: %d words unsupported (at most max_pos = %d positions, and 1024)", words,
                      w->max_pos);
    // ... and the train-mode attention kernel keeps a whole head in LDS (bert_drop.hip): refused here, before any launch, never a silent fall-back
    IISAN_CHECK_SHAPE(!(dropping && words > 224), "bert dropout: no train-mode attention kernel past 224 words, titles of %d words run in eval mode only "
                      "(drop == NULL or both probabilities 0)", words);
    const int D = w->hidden, F = w->mlp, T = words;
    const int64_t Mc = (chunk_items > 0 && chunk_items < M) ? chunk_items : M;
    WsCarver c(ws, ws_bytes);
    EncBufs b;
    carve(c, b, Mc * T, Mc, D, F, Mc * T);
    if (c.overflow || !ws) {
        iisan_set_error("bert_forward_taps: workspace too small (%zu < %zu)", ws_bytes, c.off);
        return IISAN_EWORKSPACE;
    }
    const int dt = w->dtype16;
    const bool f1blk = f1_blk32(dt, D, F, M, Mc, T, nullptr, EPI_OUT16, nullptr);      // F1 of the all-token blocks block-major
    for (int64_t m0 = 0; m0 < M; m0 += Mc) {
        const int64_t mc = (M - m0 < Mc) ? M - m0 : Mc;
        const int64_t tok = mc * T;
        float* tp = taps + m0 * n_taps * D;
        const bool mixed = !g_resid32;
        // post-LN tower: the stream IS the LayerNorm output.  resid32: X fp32 [tok, D]; mixed: Xc fp32 (CLS rows) + X16 fp16.  With fp16
        // operands the 16-bit image the products read and the fp16 stream are the same values: one buffer, written once (g_ln_fold; the add +
        // LayerNorm kernels move 6 instead of 8 bytes per element)
        const bool alias = mixed && dt == IISAN_F16 && g_ln_fold;
        void* IMG = alias ? b.X16 : b.H;
        // train mode: the keep functor of a hidden site, local row r of the launch = token row r0 + r * rs of the whole call; eval: null
        RowKeep rk;
        auto keep = [&](int site, int64_t r0, int rs) -> const RowKeep* {
            if (!dropping) return nullptr;
            rk = RowKeep{make_drop(seed, site, hp), r0, rs};
            return &rk;
        };
        if (index) IISAN_TRY(launch_bert_embed_ln_indexed(dt, text, rows, index + m0, w->word_emb, w->pos_emb, w->type_emb, w->emb_ln_w, w->emb_ln_b,
                                                          w->eps, mixed ? nullptr : b.X, IMG, b.KB, mc, T, w->vocab, D, s, b.X16, b.Xc, keep(0, m0 * T, 1)));
        else IISAN_TRY(launch_bert_embed_ln(dt, text + m0 * 2 * words, w->word_emb, w->pos_emb, w->type_emb, w->emb_ln_w, w->emb_ln_b,
                                            w->eps, mixed ? nullptr : b.X, IMG, b.KB, mc, T, w->vocab, D, s, b.X16, b.Xc, keep(0, m0 * T, 1)));
        auto tap = [&](int k) { return mixed ? launch_gather_cls(b.Xc, tp, mc, 1, D, n_taps, k, s) : launch_gather_cls(b.X, tp, mc, T, D, n_taps, k, s); };
        // x = LN(x + delta): stream and 16-bit image out
        auto add_ln = [&](const float* g, const float* be, int site) {
            return mixed ? launch_layernorm768_mixed(dt, MX_D1 | MX_LN | MX_RESY | (alias ? MX_ALIAS : 0), nullptr, b.X16, b.Xc, b.D16, nullptr, g, be, w->eps, IMG, mc, T, D, s,
                                                     nullptr, keep(site, m0 * T, 1))
                         : launch_add_layernorm768(dt, b.X, b.D16, g, be, w->eps, nullptr, b.H, b.X, tok, D, s);
        };
        int k = tap_index(tap_layers, n_taps, 0);
        if (k >= 0) IISAN_TRY(tap(k));
        const bool full_blocks = g_full_blocks || w->full_blocks;
        const int live = full_blocks ? w->layers : max_tap(tap_layers, n_taps);     // see the ViT executor
        for (int l = 0; l < live; ++l) {
            const iisan_layer_weights& L = w->layer[l];
            // a = LN(x + O(attn(x)))
            if (l + 1 < live || full_blocks) {
                IISAN_TRY(gemm(dt, EPI_QKVH16, IMG, D, L.qkv_w, L.qkv_b, b.QKV, 3 * D, nullptr, tok, s, nullptr, 0, T, w->heads));
                if (dropping) IISAN_TRY(launch_attention16_drop(dt, b.QKV, b.KB, b.H, mc, T, w->heads, make_drop(seed, 1 + 3 * l, ap), m0, false, nullptr, s));
                else IISAN_TRY(launch_attention16(dt, b.QKV, b.KB, b.H, mc, T, w->heads, s));
                IISAN_TRY(gemm(dt, EPI_OUT16, b.H, D, L.o_w, L.o_b, b.D16, D, nullptr, tok, s));
                IISAN_TRY(add_ln(L.ln1_w, L.ln1_b, 2 + 3 * l));
                // x = LN(a + FC2(gelu(FC1 a)))
                IISAN_TRY(gemm_fc1(dt, IMG, D, L.fc1_w, L.fc1_b, nullptr, b.F1, F, tok, f1blk, s));
                IISAN_TRY(gemm_fc2(dt, b.F1, F, L.fc2_w, L.fc2_b, b.D16, D, tok, f1blk, s));
                IISAN_TRY(add_ln(L.ln2_w, L.ln2_b, 3 + 3 * l));
                k = tap_index(tap_layers, n_taps, l + 1);
                if (k >= 0) IISAN_TRY(tap(k));
            } else {
                // post-LN tower: the block input H is the 16-bit image of X, so the CLS rows of H are gathered directly
                void* Hc = b.Cls;
                void* Qc = (char*)b.Cls + (size_t)b.Mcp * D * 2;
                IISAN_TRY(launch_gather_rows16(IMG, Hc, mc, T, D, s));
                IISAN_TRY(kv_all_q_cls(dt, L, IMG, b.QKV, Hc, Qc, tok, mc, T, w->heads, D, s));
                float* Xc = (float*)b.QKV;
                if (dropping) IISAN_TRY(launch_attention16_drop(dt, b.QKV, b.KB, b.H, mc, T, w->heads, make_drop(seed, 1 + 3 * l, ap), m0, true, Qc, s));
                else IISAN_TRY(launch_attention_cls16(dt, b.QKV, b.KB, b.H, mc, T, w->heads, s, Qc));
                IISAN_TRY(gemm(dt, EPI_OUT16, b.H, D, L.o_w, L.o_b, b.D16, D, nullptr, mc, s));
                if (mixed) IISAN_TRY(launch_gather_cls(b.Xc, Xc, mc, 1, D, 1, 0, s)); else IISAN_TRY(launch_gather_cls(b.X, Xc, mc, T, D, 1, 0, s));
                // (train mode: the masks of token row t = 0 of the all-token execution — compact row r is token row (m0 + r) T)
                IISAN_TRY(launch_add_layernorm768(dt, Xc, b.D16, L.ln1_w, L.ln1_b, w->eps, nullptr, b.H, Xc, mc, D, s, keep(2 + 3 * l, m0 * T, T)));
                IISAN_TRY(gemm(dt, EPI_GELU16, b.H, D, L.fc1_w, L.fc1_b, b.F1, F, nullptr, mc, s));
                IISAN_TRY(gemm(dt, EPI_OUT16, b.F1, F, L.fc2_w, L.fc2_b, b.D16, D, nullptr, mc, s));
                IISAN_TRY(launch_add_layernorm768(dt, Xc, b.D16, L.ln2_w, L.ln2_b, w->eps, nullptr, nullptr, Xc, mc, D, s, keep(3 + 3 * l, m0 * T, T)));
                k = tap_index(tap_layers, n_taps, live);
                IISAN_TRY(launch_gather_cls(Xc, tp, mc, 1, D, n_taps, k, s));
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
