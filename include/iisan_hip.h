/*
 * iisan_hip.h — C ABI of libiisan_hip.so: the MI355X (gfx950) implementation of IISAN's data-parallel hot path.
 *
 * The reference (GAIR-Lab/IISAN) has no FFI: its "operator interface" for this path is the Python nn.Module
 * surface of the Code_Uncached and Code_Cached model/ packages.  Each entry point below replaces the arithmetic of one reference
 * forward (or the autograd backward PyTorch derives from it); the reference lines are cited per function.
 * `iisan_amd/` binds these with ctypes behind modules of the same names.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer to row-major contiguous memory owned by the caller (16-byte aligned),
 *     except arguments documented as "host";
 *   - the library never allocates device memory, never synchronises and never owns buffers: scratch comes in
 *     through `ws`/`ws_bytes`, sized by the matching *_ws_bytes() query;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*); functions are re-entrant per stream;
 *   - return 0 on success, IISAN_EBADSHAPE / IISAN_EWORKSPACE / IISAN_EHIP (<0) otherwise, with a message in
 *     iisan_last_error() (thread local);
 *   - `dtype16` selects the 16-bit MFMA operand type of the frozen encoders: IISAN_F16 (default; the reference
 *     itself runs them under fp16 autocast, Code_Uncached/run.py:409) or IISAN_BF16.  Accumulation, the
 *     residual stream, LayerNorm/softmax statistics, taps and everything trainable are fp32.
 */
#ifndef IISAN_HIP_H
#define IISAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IISAN_OK 0
#define IISAN_EBADSHAPE (-1)
#define IISAN_EWORKSPACE (-2)
#define IISAN_EHIP (-3)

#define IISAN_F16 0
#define IISAN_BF16 1
#define IISAN_F32 2   /* storage type of a packed tap store only (iisan_gather_taps) */

#define IISAN_MAX_LAYERS 48
#define IISAN_MAX_SIDE 16

const char* iisan_version(void);
const char* iisan_arch(void);            /* "gfx950" */
const char* iisan_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Frozen encoders (no-grad).  Weights are packed once by the host (iisan_amd/encoders.py): matrices in the 16-bit
 * operand type, [out,in] row-major exactly like torch.nn.Linear.weight; vectors in fp32.
 * Hidden size D = 64 * heads with D = 768 (ViT-B/16, BERT-base: 12 heads) or D = 1024 (ViT-L/16, BERT-large: 16 heads), or one of the
 * narrow towers' D = 128 (BERT-tiny: 2 heads), 192 (ViT-tiny: 3), 256 (BERT-mini: 4), 384 (ViT-small: 6).  The ViT executor alone also takes
 * ViT-H/14: D = 1280 as 16 heads of 80, 14-pixel patches (below).  Any other width or pair (512; 1280 with 20 heads; 1280 on the BERT
 * executor) is IISAN_EBADSHAPE before any launch.  The taps are D wide — the tower's own width, not the side network's.
 * Every D other than 768 runs on the LayerNorm-image route of both executors (mixed fp16 / fp32-CLS residual stream; dev switch
 * resid32 works too), in eval mode only (iisan_bert_forward_taps_dropout: drop == NULL or both probabilities 0).  The
 * LayerNorm-folded route of the ViT executor (folded weights, stream epilogues, block-major stream) is 768 wide only: at any other D
 * iisan_vit_fold_bytes is 0, `folded` is ignored, and the dev switch ln_fold selects nothing.
 * ViT-H/14 (hidden 1280, heads 16): the QKV product is a plain row-major one and the attention of every block is iisan_attention16_hd80
 * (csrc/attn16_hd80.hip); the tower has NO CLS-only form of the last live block — that block runs on every token like the others (1 / 32
 * of a 32-layer tower; blocks past the deepest tap are still not run) — and iisan_encoder_plan says so (bit 32).
 * Patch sides: the multiples of 8, and 14 (any other side is IISAN_EBADSHAPE).  At 14 the patch vector of C*P*P (588) elements is
 * zero-padded to the next multiple of 64 (640) in the patch matrix, and patch_w must carry the same padding: [D, 640] with columns
 * 588..639 zero (iisan_amd/encoders.py pads it).
 * CLIP vision towers (HF CLIPVisionModel: ViT-B/32, ViT-B/16, ViT-L/14 and the toy shapes between) are ViT towers with the trailing fields
 * of iisan_vit_weights set: a LayerNorm between the embeddings and block 0 (pre_ln_w / pre_ln_b: hidden state 0, i.e. tap 0, is ITS output),
 * quick-GELU in the MLP (act = 1; the LAION checkpoints keep act = 0), no bias on the patch convolution (patch_b = NULL), eps 1e-5.  The
 * opening step is one kernel (csrc/rowops.hip, clip_open_kernel: embeddings -> pre-LayerNorm -> stream, and LN1 of block 0), the FC1
 * products run the epilogue mode 8 (EPI_QGELU16) on the 128x128 and the 256x256 kernel.  A CLIP tower — pre_ln_w != NULL or act != 0 —
 * runs on the LayerNorm-image route at every width, 768 included: iisan_vit_fold_bytes is 0 for it, `folded` is ignored and the dev switch
 * ln_fold selects nothing, as for every D != 768 (the folded route has no opening step with a pre-LayerNorm and no quick-GELU twin of its
 * FC1 epilogue).  Everything else — widths, head widths, patch sides, token counts, the CLS-only last block, chunk_items, the three entry
 * points, both operand types — is as for a ViT, and so are the refusals.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const void* qkv_w;  const float* qkv_b;   /* [3D,D] 16-bit, [3D]  (q;k;v stacked)                          */
    const void* o_w;    const float* o_b;     /* [D,D], [D]                                                     */
    const void* fc1_w;  const float* fc1_b;   /* [F,D], [F]                                                     */
    const void* fc2_w;  const float* fc2_b;   /* [D,F], [D]                                                     */
    const float* ln1_w; const float* ln1_b;   /* ViT: layernorm_before;  BERT: attention.output.LayerNorm       */
    const float* ln2_w; const float* ln2_b;   /* ViT: layernorm_after;   BERT: output.LayerNorm                 */
    /* OPTIONAL fp32 masters of qkv_w / fc1_w (null = none).  The ViT executor with fp16 operands folds LayerNorm 1 / 2 into
     * these two matrices at the start of every call (gamma-scaled, centred rows); given the masters it rounds the
     * folded rows to fp16 ONCE instead of re-rounding the 16-bit copies (tap error against the reference 1.09e-3 -> see DESIGN). */
    const float* qkv_w32; const float* fc1_w32;
} iisan_layer_weights;

typedef struct {
    int32_t hidden, layers, heads, mlp;       /* D, L, H, F                                                     */
    int32_t image, patch, channels;           /* 224, 16, 3                                                     */
    int32_t dtype16;
    float   eps;
    int32_t full_blocks;                      /* dead-work policy, see below: 0 = default, 1 = every block on every token */
    const void*  patch_w;                     /* [D, C*P*P] 16-bit (Conv2d kernel flattened (c,py,px)); P % 8 != 0: rows zero-padded to a multiple of 64 */
    const float* patch_b;                     /* [D]; NULL = no bias (CLIP)                                     */
    const float* cls_token;                   /* [D]                                                            */
    const float* pos_emb;                     /* [T, D], T = (image/patch)^2 + 1                                */
    iisan_layer_weights layer[IISAN_MAX_LAYERS];
    /* OPTIONAL (null = none): the LayerNorm-folded QKV / FC1 weights of every layer, filled ONCE by iisan_vit_fold_layernorm into a
     * caller-owned device buffer of iisan_vit_fold_bytes() bytes.  Without it every forward call folds them again into its workspace
     * (300 MB of traffic, ~0.1 ms for ViT-B; the result is the same). */
    const void* folded;
    /* ---- CLIP vision towers; all zero = the ViT above ---- */
    const float* pre_ln_w; const float* pre_ln_b;   /* [D] LayerNorm between the embeddings and block 0 (HF pre_layrnorm); NULL = none   */
    int32_t act;                              /* MLP activation: 0 = erf-GELU, 1 = quick-GELU x * sigmoid(1.702 x)                     */
    /* OPTIONAL per-channel statistics of the uint8 entry points (3 channels): all zero (default) = the reference's transform,
     * (p / 255 - .5) / .5, the code path and the bits of a struct without these fields; otherwise (p / 255 - norm_mean[c]) / norm_std[c]
     * in fp32 inside the patch-extraction kernel, every norm_std non-zero (else IISAN_EBADSHAPE) — taps identical to the fp32 entry point
     * fed with the image normalised that way on the host.  A padding slot of the indexed entry stays the all-zero normalised image.
     * The fp32 entry point takes normalised pixels and does not read them. */
    float norm_mean[3]; float norm_std[3];
} iisan_vit_weights;

typedef struct {
    int32_t hidden, layers, heads, mlp;
    int32_t vocab, max_pos;
    int32_t dtype16;
    float   eps;
    int32_t full_blocks;                      /* as in iisan_vit_weights                                        */
    const float* word_emb;                    /* [V, D] fp32 (gather only)                                      */
    const float* pos_emb;                     /* [max_pos, D]                                                   */
    const float* type_emb;                    /* [2, D] (row 0 used)                                            */
    const float* emb_ln_w; const float* emb_ln_b;
    iisan_layer_weights layer[IISAN_MAX_LAYERS];
    /* ---- DeBERTa-v2/v3 towers (HF DebertaV2Model: relative_attention, share_att_key, pos_att_type c2p|p2c, norm_rel_ebd = layer_norm,
     * position_biased_input = False, type_vocab_size = 0); all zero = the BERT above.  rel_emb != NULL makes the struct a DeBERTa tower:
     * pos_emb / type_emb are then NULL and are not read, hidden state 0 is LayerNorm(word_emb[id]) * mask, and every block's attention is
     * iisan_attention16_disent (csrc/attn16_disent.hip).  The rest of the block is BERT's post-LN block — all three entry points, chunk_items,
     * full_blocks, both operand types and the dev switch resid32 work as for BERT.  IISAN_EBADSHAPE before any launch: words > span / 2 (there
     * HF's log-bucket map of relative positions stops being the identity; no approximation is attempted) or words > 128; span < 1 or
     * span > 256; any non-zero dropout probability (iisan_bert_forward_taps_dropout: the tower is eval only, like every non-768 BERT); a
     * hidden size outside the BERT executor's set; rel_ln_w / rel_ln_b missing, or pos_emb / type_emb set beside rel_emb. ---- */
    const float* rel_emb;                     /* [2 span, D] fp32: encoder.rel_embeddings.weight                */
    const float* rel_ln_w; const float* rel_ln_b;   /* [D]: encoder.LayerNorm, applied to the table once         */
    int32_t span;                             /* position_buckets: 1 .. 256; titles of at most span / 2 (and 128) words */
    /* OPTIONAL (null = none): the projected tables of every layer, filled ONCE by iisan_deberta_rel_project into a caller-owned device
     * buffer of iisan_deberta_rel_bytes() bytes.  Without it every forward call projects them again into its workspace
     * (iisan_bert_forward_taps_ws_bytes grows by that much for such a struct only; the result is the same). */
    const void* rel_proj;
} iisan_bert_weights;

/* The position tables of a DeBERTa tower, projected by every layer's own query / key matrices (HF: pos_key_layer = key_proj(rel),
 * pos_query_layer = query_proj(rel), rel = LayerNorm(rel_embeddings.weight)).  Layout of `out`, 16-bit in the tower's operand type:
 *     [layers][heads][3][2 span][64]      third 0 = PQ = query_proj(rel), third 1 = PK = key_proj(rel), third 2 = value_proj(rel) (unused)
 * — per layer the head-major QKV image of ONE pseudo-item of 2 span tokens, written by the QKV epilogue of iisan_gemm16 itself; row d of a
 * table belongs to the relative position i - j = d - span.  `ws`: iisan_deberta_rel_ws_bytes() bytes (the 16-bit LayerNorm image of the table,
 * padded to a GEMM row tile).  IISAN_EBADSHAPE before any launch: no rel_emb / rel_ln_w / rel_ln_b, span outside 1 .. 256, an unsupported
 * hidden size; IISAN_EWORKSPACE: out == NULL or a workspace that is too small. */
size_t iisan_deberta_rel_bytes(const iisan_bert_weights* w);
size_t iisan_deberta_rel_ws_bytes(const iisan_bert_weights* w);
int iisan_deberta_rel_project(const iisan_bert_weights* w, void* out, void* ws, size_t ws_bytes, void* stream);

/* Replaces Vit_Encoder.forward + `[:,0]` tap selection (Code_Uncached/model/encoders.py:29-31, model.py:210,212):
 * images fp32 [M,C,R,R] -> taps fp32 [M, n_taps, D], taps[:,k] = CLS row of hidden state tap_layers[k]
 * (0 = embeddings, l = output of layer l; the last one is before the final LayerNorm).  `tap_layers` is a host
 * array.  `chunk_items` (0 = whole batch) bounds the activation working set. */
/* The folded weights of `w` (LayerNorm 1 / 2 of every layer folded into qkv_w / fc1_w: gamma-scaled, centred, fp16, rounded
 * sum-preservingly from the fp32 masters when the layer has them, + the folded biases): [layers][(3D + F) x D] fp16, then
 * [layers][3D + F] fp32.  0 bytes when the executor would not use them (bf16 operands; any hidden size other than 768; a CLIP tower). */
size_t iisan_vit_fold_bytes(const iisan_vit_weights* w);
int iisan_vit_fold_layernorm(const iisan_vit_weights* w, void* folded, size_t bytes, void* stream);
/* fp16 operands (dtype16 = IISAN_F16), production sizes: the executor folds LayerNorm 1 / 2 of every block into the QKV / FC1
 * weights at the start of the call (workspace: +99 MB for ViT-B) and runs no LayerNorm / residual-add kernel inside blocks 1..L-1
 * (DESIGN 6g); the taps stay inside the same tolerance against the reference (tests/test_gpu_encoders.py). */
size_t iisan_vit_forward_taps_ws_bytes(const iisan_vit_weights* w, int64_t M, int64_t chunk_items);
int iisan_vit_forward_taps(const iisan_vit_weights* w, const float* images, int64_t M,
                           const int32_t* tap_layers, int32_t n_taps, float* taps,
                           int64_t chunk_items, void* ws, size_t ws_bytes, void* stream);
/* The same from RAW uint8 pixels [M,C,R,R] (0..255): ToTensor + Normalize(.5,.5) of the reference's transform
 * (Code_Uncached/data_utils/dataset.py:46-50) are applied in fp32 inside the patch-extraction kernel — taps identical to
 * the fp32 entry point fed with the normalised image, a quarter of the input bytes. */
int iisan_vit_forward_taps_u8(const iisan_vit_weights* w, const uint8_t* images, int64_t M,
                              const int32_t* tap_layers, int32_t n_taps, float* taps,
                              int64_t chunk_items, void* ws, size_t ws_bytes, void* stream);
/* The same from a DEVICE-RESIDENT raw catalogue uint8 [rows, C, R, R]: the image of slot m is row index[m] (index int64 [M] on the
 * device), read inside the patch-extraction kernel — no [M,C,R,R] tensor exists.  This is the per-slot lookup of
 * Build_MM_Dataset.__getitem__ (Code_Uncached/data_utils/dataset.py:56-86) moved onto the device.  Any index value outside
 * [0, rows) — negative or >= rows — is a PADDING slot: never dereferenced, the tower sees the all-zero normalised image the
 * reference ships for pad slots (dataset.py:73; no uint8 pixel normalises to 0, so the zero is not a catalogue row).  A bad
 * index therefore cannot fault and needs no synchronisation to report.  Patch matrices, hence taps, are bit-identical to
 * iisan_vit_forward_taps fed with normalise(catalogue[index]) and zeros on pad slots.  Workspace: iisan_vit_forward_taps_ws_bytes.
 * IISAN_EBADSHAPE before any launch: rows <= 0, null catalogue / index, image % 8 != 0, M <= 0. */
int iisan_vit_forward_taps_u8_indexed(const iisan_vit_weights* w, const uint8_t* catalogue, int64_t rows,
                                      const int64_t* index, int64_t M,
                                      const int32_t* tap_layers, int32_t n_taps, float* taps,
                                      int64_t chunk_items, void* ws, size_t ws_bytes, void* stream);

/* Replaces Text_Encoder/Bert_Encoder.forward + tap selection (encoders.py:81-91,148-159, model.py:211,213):
 * text int64 [M, 2W] (W ids then W attention-mask values) -> taps fp32 [M, n_taps, D]. */
size_t iisan_bert_forward_taps_ws_bytes(const iisan_bert_weights* w, int64_t M, int32_t words, int64_t chunk_items);
int iisan_bert_forward_taps(const iisan_bert_weights* w, const int64_t* text, int64_t M, int32_t words,
                            const int32_t* tap_layers, int32_t n_taps, float* taps,
                            int64_t chunk_items, void* ws, size_t ws_bytes, void* stream);
/* The same from a DEVICE-RESIDENT table int64 [rows, 2W]: the text of slot m is row index[m] (the title lookup of
 * Build_MM_Dataset.__getitem__, Code_Uncached/data_utils/dataset.py:56-86, on the device).  An index value outside [0, rows) is a
 * padding slot: never dereferenced, all-zero ids and mask (dataset.py:79-84).  Taps bit-identical to iisan_bert_forward_taps fed
 * with table[index] and zero rows on pad slots.  Workspace: iisan_bert_forward_taps_ws_bytes.
 * IISAN_EBADSHAPE before any launch: rows <= 0, null table / index, M <= 0. */
int iisan_bert_forward_taps_indexed(const iisan_bert_weights* w, const int64_t* table, int64_t rows,
                                    const int64_t* index, int64_t M, int32_t words,
                                    const int32_t* tap_layers, int32_t n_taps, float* taps,
                                    int64_t chunk_items, void* ws, size_t ws_bytes, void* stream);

/* TRAIN-MODE DROPOUT of the frozen BERT tower (opt-in).  The reference trains with model.train() (Code_Uncached/run.py:394), so HF's
 * BertModel applies hidden_dropout_prob / attention_probs_dropout_prob on every training step; the entry points above are eval mode.
 * Masks are counter-based: the keep factor (0 or 1 / (1 - p)) of an element is a pure function of (seed, site, index) — the same
 * generator as iisan_sasrec_cfg's — with one 64-bit seed per forward call and
 *   site 0        embeddings:                    drop(LayerNorm(word + pos + type)) — this IS hidden state 0           (hidden_p)
 *   site 1 + 3l   block l, attention:            drop(softmax(Q K^T / 8 + key_bias)) V, no renormalisation             (attn_p)
 *   site 2 + 3l   block l, attention output:     LayerNorm(drop(dense(ctx)) + x)                                       (hidden_p)
 *   site 3 + 3l   block l, FFN output:           LayerNorm(drop(dense(gelu(..))) + a)                                  (hidden_p)
 *   hidden sites:     index = (m T + t) D + c                   (T = words, D = hidden, c = column)
 *   attention sites:  index = ((m H + h) T + q) T + k           (H = heads, q / k = query / key token)
 * where m = 0 .. M-1 is the slot's position in the WHOLE call — not within a chunk of `chunk_items`, and on the indexed route not the
 * row of the table.  Chunked and unchunked, indexed and direct calls therefore draw the same masks, and the CLS-only last live block
 * draws the masks of row t = 0 / query q = 0.  Padding slots are dropped like any other (the reference does not exempt them). */
typedef struct { float hidden_p; float attn_p; uint64_t seed; } iisan_bert_dropout;
/* iisan_bert_forward_taps (index == NULL: text_or_table is the text [M, 2W], `rows` is ignored) or iisan_bert_forward_taps_indexed
 * (index != NULL) with dropout.  drop == NULL or both probabilities 0: exactly the launches and the bits of those two.  Otherwise
 * the train-mode kernels run, for both operand types — the attention kernel of csrc/bert_drop.hip, and at the hidden sites the
 * embedding and add + LayerNorm kernels of csrc/rowops.hip instantiated with a keep functor; dead-work pruning is unchanged.  Workspace:
 * iisan_bert_forward_taps_ws_bytes is sufficient.  IISAN_EBADSHAPE before any launch: a probability outside [0, 1); dropout asked for
 * under the development switch resid32 = 1, or at a hidden size other than 768 — the row kernels have no train-mode instantiation at
 * another width, and tap caches of the wide towers are built in eval mode (never a silent fall-back to eval mode). */
int iisan_bert_forward_taps_dropout(const iisan_bert_weights* w, const int64_t* text_or_table, int64_t rows,
                                    const int64_t* index, int64_t M, int32_t words,
                                    const int32_t* tap_layers, int32_t n_taps, float* taps, int64_t chunk_items,
                                    const iisan_bert_dropout* drop, void* ws, size_t ws_bytes, void* stream);

/* Dead-work policy of the two executors above (`full_blocks` of the weights struct — part of the call, not process state).
 * 0 (default): blocks deeper than the deepest tapped hidden state are not run, and in the last live block attention / O /
 * MLP / LayerNorm run for the CLS row of every item only (K and V still for all tokens): the path consumes nothing but
 * `hidden_states[i][:, 0]`, so the taps are the same values.  1 = run every block on every token exactly like HF ViTModel /
 * BertModel do (what `bench.py` measures: SURVEY 8d counts that work). */

/* ------------------------------------------------------------------------------------------------------------
 * Side network (IISANAdaptedMModel.forward, Code_Uncached/model/model.py:209-271; Cached model.py:300-349).
 * All fp32.  Parameters arrive as a host array of device pointers in the order documented at
 * iisan_amd/ops.py::SIDE_PARAM_ORDER:
 *   for tower in (cv, text, mm): for k in 0..n_side-1: fc_down.weight, fc_down.bias, fc_up.weight, fc_up.bias
 *   gates: cv[0..n), text[0..n), mm[0..n)      (each a 1-element tensor; ignored when gated == 0)
 *   fc_cv.w, fc_cv.b, fc_bert.w, fc_bert.b, fc_mm.w, fc_mm.b,
 *   head_cv.w, head_cv.b (classifier / cv_pre_fc), head_text.w, head_text.b (title.fc / bert_pre_fc),
 *   fc_mm_down.w, fc_mm_down.b
 * Gradients are written to a parallel host array of device pointers (same order), ACCUMULATING (+=) into them;
 * the caller zeroes them.
 * Gate saturation: g = sigmoid(theta / 0.1) and 1 - g are float32, as in the reference.  From theta >= 1.7 g is exactly 1 and
 * 1 - g exactly 0: the gate's own gradient (factor g (1 - g) / 0.1) is exactly 0, and in the cv / text towers
 * (F = g tap + (1 - g) state) so is every gradient that would flow back through the state, i.e. of all earlier SANBs and gates
 * of that tower.  From theta <= -1.8 1 - g is exactly 1 and g = e^(theta / 0.1) a tiny non-zero number (2e-9 at -2.0) that
 * still multiplies the tap; it becomes exactly 0, and the gate gradient with it, only from theta <= -10.4 (where the kernels'
 * exp overflows to inf and 1 / inf gives that 0).  The float32 reference behaves the same way in every one of these cases.
 * ReLU's derivative at a pre-activation of exactly 0 is 0 (torch's convention), GELU's is 0.5.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_side;           /* SANBs of the image tower (7; 6 with remove_first); also of the text tower unless versa */
    int32_t dim_cv, dim_text; /* tap widths (768, 768; Versa e.g. 1024 / 8192)                                  */
    int32_t down;             /* adapter bottleneck (64)                                                        */
    int32_t emb;              /* embedding_dim (64)                                                             */
    int32_t gated;            /* fusion_method == "gated"                                                       */
    int32_t gelu;             /* adapter_activation == "GELU"                                                   */
    int32_t remove_first;     /* args.remove_first == "TRUE": states start at taps[:,first_index] (model.py:215-218) */
    int32_t tap_stride_cv;    /* taps are [M, tap_stride, D]; tap_index[k] selects the layer of SANB k          */
    int32_t tap_stride_text;
    int32_t tap_index[IISAN_MAX_SIDE];     /* tap-axis index used by image SANB k (and text SANB k unless versa) */
    int32_t first_index;                   /* tap index that seeds the states when remove_first                */
    /* ---- Versa (Code_Cached_Asym/model/model.py:257-429); all zero for the Uncached / Cached variants ---- */
    int32_t versa;            /* 1: asymmetric towers: heads are fc_cv[E,Dc], fc_bert[E,Dt], fc_mm[d,d] then cv_pre_fc[E,E],
                                 bert_pre_fc[E,E], fc_mm_down[E,d], d = min(Dc,Dt); group layer-drop; dim-align        */
    int32_t n_side_text;      /* SANBs of the text tower                                                        */
    int32_t tap_index_text[IISAN_MAX_SIDE];
    int32_t first_index_text;
    int32_t taps_exact16;     /* 1: the caller guarantees that every tap value is exactly representable in fp16 (taps cached in fp16, as
                                 preprocess_*.py of Code_Cached_Asym writes them): the split-operand dim-align products then take the tap
                                 with scale 1, skip its amax pass and (round 6) do not build the lo plane of its image — a tap that is NOT
                                 exact in fp16 would be rounded to fp16 there.  0 = unknown (always safe)                   */
} iisan_side_cfg;

/* Parameter table (host array of device pointers), n_mm = min(n_cv, n_text):
 *   image SANBs k=0..n_cv-1:  fc_down.weight, fc_down.bias, fc_up.weight, fc_up.bias
 *   text  SANBs k=0..n_t-1 :  same          mm SANBs i=0..n_mm-1: same
 *   gates: image[n_cv], text[n_t], mm[n_mm]   (1-element tensors; ignored when gated == 0)
 *   versa && dim_cv != dim_text: dim-align down_project_list[i].weight, .bias for i=0..n_mm-1
 *   fc_cv.w,.b   fc_bert.w,.b   fc_mm.w,.b
 *   head_cv.w,.b (classifier | cv_pre_fc)   head_text.w,.b (title.fc | bert_pre_fc)   fc_mm_down.w,.b          */
int32_t iisan_side_net_num_params(const iisan_side_cfg* cfg);
size_t iisan_side_net_ws_bytes(const iisan_side_cfg* cfg, int64_t M);        /* saved activations + scratch    */
/* out: item3 fp32 [M, 3*emb] = cat[cv, text, mm] (the com_dense input, model.py:69) */
/* `fwd_token` (out, host): what the backward call needs to know about THIS forward call — which kernel routes filled the
 * workspace.  The caller carries it to iisan_side_net_bwd together with the workspace (the library keeps no per-call state:
 * SURVEY 8b "stateless").  A backward call whose token does not match the routes it would take itself returns IISAN_EBADSHAPE. */
int iisan_side_net_fwd(const iisan_side_cfg* cfg, const float* taps_cv, const float* taps_text, int64_t M,
                       const void* const* params, float* item3, void* ws, size_t ws_bytes, uint64_t* fwd_token, void* stream);
int iisan_side_net_bwd(const iisan_side_cfg* cfg, const float* taps_cv, const float* taps_text, int64_t M,
                       const void* const* params, const float* d_item3, void* const* grads,
                       void* ws, size_t ws_bytes, uint64_t fwd_token, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Plain fp32 Linear (com_dense, Code_Uncached/model/model.py:36-37,69): y = x W^T + b ; bwd accumulates dW, db.
 * ---------------------------------------------------------------------------------------------------------- */
int iisan_linear_fwd(const float* x, const float* w, const float* b, float* y, int64_t M, int32_t K, int32_t N,
                     void* stream);
int iisan_linear_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db,
                     int64_t M, int32_t K, int32_t N, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * SASRec user encoder (User_Encoder.forward, Code_Uncached/model/encoders.py:60-65; modules.py:6-96).  fp32.
 * params order (host array of device pointers): position_embedding.weight, layer_norm.{weight,bias}, then per
 * block: w_Q, w_K, w_V, fc (weights), attn layer_norm.{weight,bias}, w_1.{weight,bias}, w_2.{weight,bias},
 * ffn layer_norm.{weight,bias}.   x: [B,S,E]; log_mask: [B,S]; y: [B,S,E].
 * With emb == 64, seq <= 16 and 1, 2 or 4 heads (the reference configuration is 64 / 10 / 2) each direction is ONE launch
 * (+ a fixed-order reducer of per-workgroup parameter-gradient partial sums in the backward: bit-reproducible, no atomics);
 * other shapes (seq <= 32, emb a multiple of 64 up to 256, emb / heads <= 64, 1 .. 8 blocks; anything else is IISAN_EBADSHAPE)
 * take one launch per operator.  Either way the forward keeps every intermediate the backward needs in `ws`
 * (same slots), and gradients ACCUMULATE (+=) into the caller's tensors.
 * Mask: key k is allowed for query q where k <= q and log_mask[b, k] != 0 (ANY non-zero value, not only 1); every other
 * key gets -1e9 added to score / sqrt(emb / heads), as the reference does.  A query row WITHOUT an allowed key (left padding
 * in front of the first real position, a sequence whose log_mask is all 0: the eval user without history) therefore carries
 * -1e9 on every key: while |score / sqrt(emb / heads)| < 32 the float32 sum is -1e9 exactly (the spacing at 1e9 is 64) and the
 * row attends UNIFORMLY OVER ALL `seq` POSITIONS, later ones included; beyond that it is the softmax of the float32
 * roundings of -1e9 + score, as in the reference.  Such a row's position is itself padding, a masked key for every query:
 * it never reaches a row that has an allowed key (tests/test_gpu_sasrec_regimes.py).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t seq, emb, heads, blocks;       /* 10, 64, 2, 2                                                     */
    float   dropout;                        /* 0 => identity (eval)                                             */
    uint64_t seed;                          /* dropout stream (ignored when dropout == 0)                       */
} iisan_sasrec_cfg;

size_t iisan_sasrec_ws_bytes(const iisan_sasrec_cfg* cfg, int64_t B);
int iisan_sasrec_fwd(const iisan_sasrec_cfg* cfg, const float* x, const float* log_mask, int64_t B,
                     const void* const* params, float* y, void* ws, size_t ws_bytes, void* stream);
int iisan_sasrec_bwd(const iisan_sasrec_cfg* cfg, const float* x, const float* log_mask, int64_t B,
                     const void* const* params, const float* dy, float* dx, void* const* grads,
                     void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * In-batch debiased cross-entropy (ModelMM.forward, Code_Uncached/model/model.py:81-104), fused: the [T,M]
 * logits are never materialised.  ids int64 [bs*(S+1)], score fp32 [bs*(S+1),E], prec fp32 [bs*S,E],
 * log_mask fp32 [bs,S], pop_prob fp32 [n_pop = item_num+1].  loss: 1 float.  row_lse: [bs*S] scratch kept for bwd.
 * The library never syncs, so a bad INPUT VALUE cannot come back as a return code: an id outside [0, n_pop) is
 * not dereferenced and makes the loss NaN (the reference would raise an IndexError at model.py:63).
 * Ids repeated inside a sequence and log_mask values other than 0 / 1 follow the reference: a position counts where log_mask != 0, a
 * column whose id occurs anywhere in the row's own sequence is filled with -1e4 and only the label column is spared — unless the label
 * column is itself history padding (log_mask == 0 there), which keeps the fill and carries no gradient (tests/test_gpu_ce_regimes.py).
 * From 2^24 logits on (bs = 1024: 10,240 x 11,264) the two passes run on the 16-bit matrix cores with score / prec split
 * into fp16 hi + lo planes (csrc/ce.hip ce16_*: the accuracy of an fp32 product to ~2^-22; the workspace also holds the
 * operand images and the per-range partial results: ~95 MB at bs = 1024); below, on the f32-input matrix cores.
 * Limits (IISAN_EBADSHAPE otherwise, before any launch): bs > 0, 1 <= S <= 63, E in {64, 128, 192, 256} (the multiples of 64 up to 256, as
 * iisan_sasrec_*).  E > 64 runs on the f32-input matrix cores at every size (the split-operand passes are 64 wide), and its workspace
 * holds no operand images: iisan_inbatch_ce_ws_bytes_e(bs, S, E), 10.7 MB at bs = 1024, S = 10, E = 256.
 * iisan_inbatch_ce_ws_bytes(bs, S) is iisan_inbatch_ce_ws_bytes_e(bs, S, 64); _ws_bytes_e returns 0 for a shape outside the limits.
 * ---------------------------------------------------------------------------------------------------------- */
size_t iisan_inbatch_ce_ws_bytes(int64_t bs, int32_t S);
size_t iisan_inbatch_ce_ws_bytes_e(int64_t bs, int32_t S, int32_t E);
int iisan_inbatch_ce_fwd(const int64_t* ids, const float* score, const float* prec, const float* log_mask,
                         const float* pop_prob, int64_t n_pop, int64_t bs, int32_t S, int32_t E, float* loss,
                         void* ws, size_t ws_bytes, uint64_t* fwd_token, void* stream);
/* d_loss: host scalar multiplier (upstream gradient).  d_score [M,E] and d_prec [T,E] are overwritten.  `fwd_token`: the value
 * the forward call on this workspace returned (it says whether that call left d_prec for d_loss = 1 in the workspace, which
 * this call then only scales); 0 or a token of another call shape (bs, S or E) is IISAN_EBADSHAPE. */
int iisan_inbatch_ce_bwd(const int64_t* ids, const float* score, const float* prec, const float* log_mask,
                         const float* pop_prob, int64_t bs, int32_t S, int32_t E, float d_loss,
                         float* d_score, float* d_prec, void* ws, size_t ws_bytes, uint64_t fwd_token, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Eval scoring (eval_model + metrics_topK, Code_Uncached/data_utils/metrics.py:59-67,198-207): for each user
 * the 1-based rank of `target` among items 1..item_num by score = prec . item_emb, history scored -inf, ties
 * towards the lower item id.  history: int32 [U, hist_stride] padded with 0.  ranks: int32 [U]; a target outside
 * 1..item_num is not dereferenced and yields rank -1, history ids outside that range are ignored.
 * Limits (IISAN_EBADSHAPE otherwise): E in {64, 128, 192, 256}, hist_stride <= 256 (the history correction of a user lives in LDS),
 * prec and item_emb 16-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
int iisan_score_rank(const float* prec, const float* item_emb, int64_t U, int64_t n_items_plus1, int32_t E,
                     const int32_t* history, int32_t hist_stride, const int32_t* target, int32_t* ranks,
                     void* stream);

/* The recommendation list itself (north_star "top-k indices"; SURVEY 8b `score_topk`): topk_ids int32 [U, k] = the first k item ids
 * of `order = torch.argsort(y_score, descending=True)` in metrics_topK (Code_Uncached/data_utils/metrics.py:59-60) over the row
 * eval_model builds at metrics.py:198-206 (history scored -inf, column 0 dropped, id = position + 1), ties towards the lower item id
 * (= a stable descending argsort; the reference leaves tie order unspecified).  Scores come out of the same MFMA chain as
 * iisan_score_rank's: a target that call ranks r <= k sits at topk_ids[u, r-1].  topk_scores fp32 [U, k] (nullable): the scores of
 * those items.  history ids outside 1..item_num are ignored, any hist_stride >= 0 is accepted.  When fewer than k items remain outside
 * a user's history the trailing slots hold id 0 / score -inf (the reference's argsort lists the -inf items there).
 * Limits (IISAN_EBADSHAPE otherwise): E in {64, 128, 192, 256}, 1 <= k <= 16, prec and item_emb 16-byte aligned; workspace from
 * iisan_score_topk_ws_bytes (the same at every width; 0 bytes when one workgroup per 32 users covers the whole catalogue). */
size_t iisan_score_topk_ws_bytes(int64_t U, int64_t n_items_plus1, int32_t k);
int iisan_score_topk(const float* prec, const float* item_emb, int64_t U, int64_t n_items_plus1, int32_t E,
                     const int32_t* history, int32_t hist_stride, int32_t k, int32_t* topk_ids, float* topk_scores,
                     void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device-resident user store: the user side of a batch built on the device (csrc/users.hip) — what
 * Code_Uncached/data_utils/dataset.py:65-92 (train) and :183-189 (eval) build per user on the host.  User sequences live in CSR form:
 * seq_off int64 [n_users + 1], seq_items int32 [nnz] (item ids 1..item_num); exclusion lists in a second CSR of the same form.
 * user_index int64 [B] on the device names the batch's users, duplicates and any order allowed; a value outside [0, n_users) is a PADDING
 * ROW: nothing of the store is read for it and its ids, mask, target and history are all zero (iisan_score_rank then reports -1 for it,
 * as for any invalid target).  With L the length of a user's sequence:
 * ---------------------------------------------------------------------------------------------------------- */
#define IISAN_WIN_TRAIN 0   /* ids [B, S+1]: the last min(L, S+1) items right-aligned, zeros in front;
                               log_mask[b, j] = 1 for j >= S+1-min(L, S+1), j < S   (dataset.py:66-72)                              */
#define IISAN_WIN_EVAL  1   /* sequence = inputs + target: target[b] = last item; ids [B, S] = the min(L-1, S) items before it,
                               right-aligned; log_mask 1 on them   (dataset.py:183-189)                                             */
#define IISAN_WIN_INPUT 2   /* every item is an input: ids [B, S] = the last min(L, S), log_mask 1 on them; no target               */
/* ids int64, log_mask fp32 [B, S] (every mode), target int32 [B]: required in EVAL mode, optional otherwise (written 0 when given).
 * x (nullable; EVAL / INPUT modes only) fp32 [B, S, E]: x[b, j] = item_emb[ids[b, j]] for item_emb fp32 [n_items_plus1, E] — a padded
 * position copies ROW 0 of the table (what indexing the table with the padded ids gives), an id outside [0, n_items_plus1) is not
 * dereferenced and yields a zero row.  Every element of every output given is written.
 * Limits (IISAN_EBADSHAPE before any launch, the message names the argument): B >= 1, 1 <= S <= 63, no null pointer among those the mode
 * needs, x only with item_emb and not in TRAIN mode, E % 4 == 0, item_emb and x 16-byte aligned. */
int iisan_user_windows(const int64_t* seq_off, const int32_t* seq_items, int64_t n_users,
                       const int64_t* user_index, int64_t B, int32_t S, int32_t mode,
                       int64_t* ids, float* log_mask, int32_t* target,
                       const float* item_emb, int64_t n_items_plus1, int32_t E, float* x, void* stream);
/* history int32 [B, hist_stride] = the first min(len, hist_stride) entries of each user's exclusion list, padded with 0 — the `history`
 * operand of iisan_score_rank / iisan_score_topk.  B >= 1, hist_stride >= 1. */
int iisan_user_history(const int64_t* hist_off, const int32_t* hist_items, int64_t n_users,
                       const int64_t* user_index, int64_t B, int32_t hist_stride, int32_t* history, void* stream);
/* counts int64 [K + 2] += histogram of ranks int32 [U] (the caller zeroes it): counts[0] ranks < 1 (invalid targets), counts[r] rank r for
 * 1 <= r <= K, counts[K + 1] ranks > K.  Integer adds only: the result does not depend on the launch's schedule.  U >= 1, 1 <= K <= 64. */
int iisan_rank_histogram(const int32_t* ranks, int64_t U, int32_t K, int64_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused Adam over a flat fp32 parameter buffer with per-segment learning rates (torch.optim.Adam defaults, the
 * optimiser of Code_Uncached/run.py:323-336).  seg_end (host, int64[n_seg]) are exclusive end offsets: element i takes
 * seg_lr[s] for the first s with i < seg_end[s].  IISAN_EBADSHAPE unless n > 0, 1 <= n_seg <= 8, step >= 1, seg_end is
 * non-decreasing from 0 (empty segments allowed) and seg_end[n_seg-1] == n, so that every element has exactly one segment.
 * ---------------------------------------------------------------------------------------------------------- */
int iisan_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end,
                    const float* seg_lr, int32_t n_seg, int32_t step, float beta1, float beta2, float eps,
                    float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Primitive kernels, exported for unit tests and micro-benchmarks only.
 * ---------------------------------------------------------------------------------------------------------- */
/* C = epilogue(A[M,K] · W[N,K]^T + bias): 16-bit operands, fp32 accumulate.
 * mode 0: out16 = acc+bias     1: out16 = gelu_erf(acc+bias)     2: out32 = acc+bias+resid32 (resid may alias out)
 * mode 8: out16 = quick_gelu(acc+bias), quick_gelu(x) = x * sigmoid(1.702 x) — wherever mode 1 is taken: the 128x128 kernel (ragged tiles
 * included) and gemm16_h256, plain or with a block-major output (iisan_gemm16_blk32).  gemm16_s256 (dev switch gemm16_variant = 3, the
 * race screen) has no mode 8: iisan_gemm16_route answers 0 there and the 128x128 kernel runs it.
 * A must be readable for ceil(M/256)*256 rows (tiles are loaded whole; rows >= M are never stored).
 * K % 64 == 0; N % 128 == 0, or N % 64 == 0 below 768 (the 192- and 576-column products of a 192-wide tower: a ragged last column
 * tile on the 128x128 kernel, W and bias read for rows / entries 0..N-1 only).  Anything else: IISAN_EBADSHAPE. */
int iisan_gemm16(int32_t dtype16, int32_t mode, const void* A, const void* W, const float* bias, void* out,
                 const float* resid, int64_t M, int32_t N, int32_t K, void* stream);
/* LayerNorm over rows of width 768: out16 (nullable) / out32 (nullable) */
int iisan_layernorm768(int32_t dtype16, const float* x, const float* g, const float* b, float eps,
                       void* out16, float* out32, int64_t rows, void* stream);
/* The same over rows of `width` elements, width 768 or 1024, or 128, 192, 256, 384, or 1280 — the row widths the encoders' row kernels are built for
 * (ViT-B / BERT-base, ViT-L / BERT-large, the narrow towers, ViT-H/14).  Any other width: IISAN_EBADSHAPE, nothing launched.  At width 768 it is the call above. */
int iisan_layernorm(int32_t dtype16, const float* x, const float* g, const float* b, float eps,
                    void* out16, float* out32, int64_t rows, int32_t width, void* stream);
/* softmax(QK^T/sqrt(64) + key_bias)V per (item, head); qkv 16-bit HEAD-MAJOR [items, H, 3 (q|k|v), S, 64] (what the QKV
 * GEMM epilogue of the encoders writes); ctx 16-bit token-major [items*S, H*64];
 * key_bias fp32 [items,S] or NULL (values < 0 mark masked keys).
 * 1 <= S <= 1024: up to 224 tokens a whole head's K and V sit in LDS (csrc/attn16.hip, attn16_dma.hip); 224 < S <= 1024 runs the
 * streaming-softmax kernel below.  S > 1024: IISAN_EBADSHAPE, nothing launched. */
int iisan_attention16(int32_t dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int32_t S,
                      int32_t heads, void* stream);
/* the same arithmetic by the streaming-softmax kernel (csrc/attn16_long.hip: keys in chunks of 128, running maximum / sum / context per
 * query row) at ANY 1 <= S <= 1024 — what iisan_attention16 launches past 224 tokens, reachable below that for tests and timing */
int iisan_attention16_long(int32_t dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int32_t S,
                           int32_t heads, void* stream);
/* 80-wide heads (ViT-H/14; csrc/attn16_hd80.hip): softmax(QK^T/sqrt(80) + key_bias)V by the same streaming softmax, 1 <= S <= 1024.
 * qkv 16-bit ROW-MAJOR [items*S, 3*H*80] — the output of a plain product: Q, K, V of head h at columns h*80, H*80 + h*80, 2*H*80 + h*80 —
 * ctx 16-bit token-major [items*S, H*80]; key_bias as in iisan_attention16.  S > 1024: IISAN_EBADSHAPE, nothing launched. */
int iisan_attention16_hd80(int32_t dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int32_t S,
                           int32_t heads, void* stream);
/* the same for the CLS query (token 0) of every item only: ctx_cls 16-bit [items, H*64].  Used by the encoder executors
 * in the last live block, where only `hidden_states[i][:, 0]` is consumed (Code_Uncached/model/model.py:210-213).
 * 1 <= S <= 1024 (a score row of 256 keys per wave up to S = 256, of 1,024 beyond); S > 1024: IISAN_EBADSHAPE, nothing launched. */
int iisan_attention_cls16(int32_t dtype16, const void* qkv, const float* key_bias, void* ctx_cls, int64_t items,
                          int32_t S, int32_t heads, void* stream);
/* Disentangled attention of DeBERTa-v2/v3 (csrc/attn16_disent.hip), per (item, head), with delta(i, j) = i - j + span:
 *     score[i][j] = (Q_i . K_j + Q_i . PK[delta] + K_j . PQ[delta]) / sqrt(3 * 64) + key_bias[j],   ctx = softmax_j(score) V
 * qkv, key_bias and ctx exactly as for iisan_attention16; `rel` = ONE layer of the iisan_deberta_rel_project image, 16-bit
 * [heads][3][2 span][64] (third 0 = PQ, third 1 = PK).  The three products accumulate in fp32 on the matrix cores; P and the context are
 * rounded to the operand type as in iisan_attention16.  1 <= S <= min(128, span) and 1 <= span <= 256 (the pairs of a title then reach rows
 * 1 .. 2 span - 1 of a table, all of them inside it); anything else is IISAN_EBADSHAPE, nothing launched. */
int iisan_attention16_disent(int32_t dtype16, const void* qkv, const void* rel, const float* key_bias, void* ctx, int64_t items,
                             int32_t S, int32_t heads, int32_t span, void* stream);
/* the same for the CLS query (token 0) of every item only — both positional indices are span - j —: ctx_cls 16-bit [items, H*64] */
int iisan_attention_cls16_disent(int32_t dtype16, const void* qkv, const void* rel, const float* key_bias, void* ctx_cls, int64_t items,
                                 int32_t S, int32_t heads, int32_t span, void* stream);
/* iisan_attention16 (cls_only == 0) / iisan_attention_cls16 (cls_only != 0; the query is token 0 of the q block) with the
 * probabilities dropped at `site` (iisan_bert_dropout; slot m = item); p = 0 gives the bits of iisan_attention16.  S <= 224. */
int iisan_attention16_dropout(int32_t dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int32_t S,
                              int32_t heads, float p, uint64_t seed, int32_t site, int32_t cls_only, void* stream);
/* fp32 MFMA GEMM: C[M,N] = op(A) op(B) (+bias)(+relu); ta: A stored [K,M]; tb: B stored [K,N] (else [N,K]);
 * accumulate != 0: C += (atomic, split-K capable) */
int iisan_gemm32(const float* A, const float* B, const float* bias, float* C, int64_t M, int32_t N, int64_t K,
                 int32_t ta, int32_t tb, int32_t relu, int32_t accumulate, void* stream);
/* The same product on the 16-bit matrix cores with split operands (csrc/split.hip): each fp32 operand becomes two fp16
 * planes (hi + lo, power-of-two scale from the tensor's amax) and  A·B^T ~= Ah·Bh^T + Ah·Bl^T + Al·Bh^T  runs as one
 * fp16 MFMA GEMM over 3K with fp32 accumulation — a few fp32 ulps from the FMA chain, ~5x the f32 matrix rate.  Used by
 * the side network for its large Linear layers (fc_* 768x768, Versa dim-align).  No activation epilogue; N % 8 == 0;
 * operands 16-byte aligned; workspace from iisan_gemm_x3_ws_bytes. */
size_t iisan_gemm_x3_ws_bytes(int64_t M, int32_t N, int64_t K);
int iisan_gemm_x3(const float* A, const float* B, const float* bias, float* C, int64_t M, int32_t N, int64_t K,
                  int32_t ta, int32_t tb, int32_t accumulate, void* ws, size_t ws_bytes, void* stream);
/* Packed device-resident tap store (replaces the 22 `torch.load` calls per sample of
 * Code_Cached/data_utils/dataset.py:29-34,77-90): table [rows, row_elems] in fp32 / fp16 / bf16 (store_dtype), row i =
 * the selected CLS taps of item i flattened ([n_sel, D]); out[m, :] = fp32(table[ids[m], :]).  ids int64 on device,
 * clamped to [0, rows); row_elems must be a multiple of 8. */
int iisan_gather_taps(int32_t store_dtype, const void* table, int64_t rows, const int64_t* ids, float* out, int64_t M,
                      int64_t row_elems, void* stream);
/* f32 -> 16-bit conversion helper used when packing weights */
int iisan_cast16(int32_t dtype16, const float* src, void* dst, int64_t n, void* stream);

/* Kernel-level entry points of the encoder GEMM's epilogue families (tests/test_gpu_primitives.py, tools/gemm_*.py): the
 * products behind HF ViTLayer's QKV / O / FC1 / FC2 dense layers as the executors launch them. */
/* iisan_gemm16 with explicit leading dimensions (mode 0 / 1) */
int iisan_gemm16_ld(int32_t dtype16, int32_t mode, const void* A, const void* W, const float* bias, void* out, int64_t M,
                    int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t ldo, void* stream);
/* fp16 operands, fp32 output, optional split-K (ksplit > 1: atomic accumulation into a caller-zeroed out) */
int iisan_gemm16_f32(const void* A, const void* W, float* out, int64_t M, int32_t N, int32_t K, int32_t ksplit,
                     void* stream);
/* LN(x) W^T + b with the LayerNorm applied in the epilogue: A = x [M,K] fp16 (the residual stream), W / bias = the folded set
 * (iisan_fold_ln_weights), rowstat [ceil(M/256)*256] = rstd per row (NULL: plain product); mode 1 (GELU) or 4 (head-major QKV,
 * S tokens per item, N / 192 heads) */
int iisan_gemm16_lna(int32_t mode, const void* A, const void* W, const float* bias, void* out, const float* rowstat, int64_t M,
                     int32_t N, int32_t K, int32_t S, void* stream);
/* gamma-folded, centred weights of one LayerNorm -> Linear pair: Wf[n,:] = fp16(g * W[n,:] - mean_k(g * W[n,:])), bf = b_lin + W beta
 * (w32 != 0: W is the fp32 master, else the 16-bit copy) */
int iisan_fold_ln_weights(const void* W, int32_t w32, const float* bias, const float* g, const float* b, void* Wf, float* bf,
                          int32_t N, void* stream);
/* x16 <- fp16(x16 + A W^T + bias) in place (fp16 residual stream, N <= 1024) + per-64-column-slice row sums / sums of squares into
 * rowpart [N/64][Mpad][2]; rows m with m % S == 0 (CLS rows) receive the delta alone */
int iisan_gemm16_stream(const void* A, const void* W, const float* bias, void* x16, float* rowpart, int64_t M, int32_t N,
                        int32_t K, int32_t S, void* stream);
/* rowpart -> rstd per row; folds the CLS rows' deltas into their fp32 stream xc [items, N] */
int iisan_stream_stats_finalize(const float* rowpart, int32_t nslots, int64_t Mpad, void* x16, float* xc, float* rstat,
                                float eps, int64_t items, int32_t Ttok, void* stream);
/* host-side predicate (no device touched): does the persistent 256x256 kernel take this product? */
int32_t iisan_gemm16_h256_applicable(int32_t mode, int64_t M, int32_t N, int32_t K, int32_t qkv_S, int32_t qkv_heads,
                                     int32_t qkv_which0);
/* host-side routing query (no device touched): the kernel family iisan_gemm16* runs this product on under the current
 * gemm16_variant — 0 = 128x128, 1 = staggered 256x256 (gemm16_s256), 2 = gemm16_h256, negative = rejected (iisan_last_error).
 * Operands with natural leading dimensions; qkv_S is the patch count of the patch modes; with_rowstat: LayerNorm in the epilogue. */
int32_t iisan_gemm16_route(int32_t dtype16, int32_t mode, int64_t M, int32_t N, int32_t K, int32_t qkv_S, int32_t qkv_heads,
                           int32_t qkv_which0, int32_t with_rowstat);
/* host-side query of the launch iisan_gemm32 / the side network makes for a group of nprob fp32 products C[M,N] = op(A) op(B) under `flags`
 * (csrc/common.h: G32_*) with scratch_floats of split-K scratch registered (no device memory touched; the plan depends on the compute-unit
 * count of the current device, 256 without one).  Natural leading dimensions, aligned operands; with_colsum: every problem wants the column
 * sums of A.  plan12 = kernel (0 tiled, 1 K = 64, 2 weight-gradient, 3 split into a K = 64 launch and a rest launch), row-tile height, K
 * splits, scratch use (0 none, 1 partials + epilogue reducer, 2 partials added to C), fast fetch, three K-tiles in flight, column sums (0 none,
 * 1 out of the product, 2 own launch), 64-column blocks per workgroup (K = 64 kernel), grid x / y / z, members of the K = 64 launch of a split.
 * Returns the kernel, negative = rejected (iisan_last_error). */
int32_t iisan_gemm32_plan(const int64_t* M, const int32_t* N, const int64_t* K, int32_t nprob, int32_t flags, int64_t scratch_floats,
                          int32_t with_colsum, int32_t* plan12);
/* host-side query: the route iisan_inbatch_ce_fwd takes for this shape under the current ce_fast — 0 generic kernel, 1 separate row passes,
 * 2 fused f32 row pass, 3 split-operand passes; negative = the shape is rejected (iisan_last_error) */
int32_t iisan_inbatch_ce_route(int64_t bs, int32_t S);
/* the same at embedding width E (iisan_inbatch_ce_route is the E = 64 call): never 3 at E > 64; -1 for a shape or width outside the limits */
int32_t iisan_inbatch_ce_route_e(int64_t bs, int32_t S, int32_t E);
/* host-side query: what iisan_vit_forward_taps* / iisan_bert_forward_taps* decide once per call, before their first launch, under the current
 * dev switches (resid32, ln_fold, blk32, full_blocks, gemm16_variant) — the executors' own decision code, asked without weights or a
 * workspace.  tokens: per item (patches + 1 / words); deepest_tap: the largest tap layer of the call; full_blocks: the weights struct's field;
 * folded: the weights struct carries a folded set (iisan_vit_fold_layernorm).  Negative = the executors refuse these sizes (iisan_last_error).
 * ViT: bits 0-1 how the residual stream is carried (0 fp32 stream of resid32, 1 mixed stream + LayerNorm images, 2 LayerNorm in the QKV / FC1
 * epilogues, 3 ... and the residual adds in the O / FC2 epilogues), 4 = the FC1 -> FC2 intermediate is block-major, 8 = the stream is, 16 = the
 * call folds the LayerNorm weights itself, 32 = 80-wide heads (hidden 1280, heads 16): row-major QKV, iisan_attention16_hd80, and the last live
 * block runs on every token instead of on the CLS rows.  IISAN_TOWER_CLIP: the ViT executor's decision for a CLIP tower (pre-LayerNorm,
 * quick-GELU FC1), the ViT bit meanings; bits 0-1 are never 2 or 3 and bits 8 and 16 never set.  BERT: 1 = mixed stream, 2 = stream and 16-bit image share one buffer, 4 = block-major FC1 -> FC2. */
#define IISAN_TOWER_VIT 0
#define IISAN_TOWER_BERT 1
#define IISAN_TOWER_CLIP 2
/* IISAN_TOWER_DEBERTA: the BERT executor's decision for a DeBERTa tower (rel_emb != NULL), the BERT bit meanings.  The last argument is then
 * the tower's `span` (position_buckets) instead of `folded`: tokens > span / 2, tokens > 128 or a span outside 1 .. 256 are refused like
 * the forward refuses them. */
#define IISAN_TOWER_DEBERTA 3
int32_t iisan_encoder_plan(int32_t tower, int32_t dtype16, int32_t hidden, int32_t heads, int32_t mlp, int32_t tokens, int64_t M,
                           int64_t chunk_items, int32_t deepest_tap, int32_t full_blocks, int32_t folded);

/* ------------------------------------------------------------------------------------------------------------
 * DEV section — process-wide development switches and measurement hooks.  NOT part of the product contract: a
 * product process calls none of these and the library defaults ARE the product routes.  Every other entry point
 * above is stateless and re-entrant per stream; these are the only process-global state the library has.
 * ---------------------------------------------------------------------------------------------------------- */
/* Named switches (kernel-family selection for golden-pinned reference runs, ablation bits, A/B routes).  Names are
 * registered by the kernel files (csrc/common.h: IISAN_DEV_KNOB); iisan_dev_state(buf, cap, 1) lists them all.
 * set: 0 or IISAN_EBADSHAPE (unknown name).  get: the value, INT64_MIN for an unknown name.
 * state: writes "name=value,..." of every switch NOT at its library default (all != 0: every switch) and returns the
 * length needed; "" means the product routes are in force.  reset: every switch back to its default.
 * Names of the form "count:<kernel family>" (round 6) are launch COUNTERS, not switches: get reads, set / reset zero them, state lists them only
 * with all != 0.  tests/test_gpu_trainable.py pins the default dispatch of the bench shapes with them. */
int32_t iisan_dev_set(const char* name, int64_t value);
int64_t iisan_dev_get(const char* name);
size_t iisan_dev_state(char* buf, size_t cap, int32_t all);
void iisan_dev_reset(void);
/* Per-launch HIP-event timing of one kernel class on the launching stream (bench.py's roofline.dominant_kernel):
 * cls 0 = off, 1 = the 16-bit encoder GEMM, 2 = the f32-matrix-core family of the trainable side.  only_stream: with on != 0
 * only launches on `stream` are timed.  collect: waits for the recorded events, returns the launch count, fills total
 * milliseconds and FLOPs; last_bytes: algorithmic bytes of the launches of the last collect. */
void iisan_timing_enable(int32_t cls);
void iisan_timing_only_stream(void* stream, int32_t on);
int64_t iisan_timing_collect(double* total_ms, double* total_flops);
double iisan_timing_last_bytes(void);
/* Block-major ("blk32") 16-bit intermediates of the persistent 256x256 GEMM (tests, tools/gemm_blk32_ab.py): a [Mpad, C]
 * matrix, Mpad % 32 == 0 and C % 32 == 0, as 32 x 32 blocks of 2 KiB; element (m, c) at byte
 *   ((m >> 5) * (C >> 5) + (c >> 5)) * 2048 + ((c >> 3) & 1) * 1024 + (((c >> 4) & 1) * 32 + (m & 31)) * 16 + (c & 7) * 2.
 * The executors' FC1 -> FC2 intermediate carries it (dev switch blk32 >= 1) and the ViT residual stream of the product route (blk32 = 2,
 * the default; 0 = row-major everywhere).  iisan_gemm16_blk32: iisan_gemm16 (mode 0 / 1 / 8; rowstat != NULL: LayerNorm in the epilogue as
 * iisan_gemm16_lna) with "A is block-major" (mode 0; mode 1 with rowstat and a block-major out: the stream into FC1) and "out is
 * block-major" (mode 1, and mode 8 without rowstat); iisan_gemm16_stream_blk32 / iisan_stream_stats_finalize_blk32: iisan_gemm16_stream and its finalize step with
 * a block-major A and / or a block-major stream x16.  Every combination or kernel route that does not carry a flag returns
 * IISAN_EBADSHAPE. */
int iisan_gemm16_blk32(int32_t dtype16, int32_t mode, const void* A, const void* W, const float* bias, void* out, const float* rowstat,
                       int64_t M, int32_t N, int32_t K, int32_t a_blk32, int32_t out_blk32, void* stream);
int iisan_gemm16_stream_blk32(const void* A, const void* W, const float* bias, void* x16, float* rowpart, int64_t M, int32_t N,
                              int32_t K, int32_t S, int32_t a_blk32, int32_t x_blk32, void* stream);
int iisan_stream_stats_finalize_blk32(const float* rowpart, int32_t nslots, int64_t Mpad, void* x16, float* xc, float* rstat, float eps,
                                      int64_t items, int32_t Ttok, int32_t x_blk32, void* stream);
/* iisan_gemm16_h256_applicable / iisan_gemm16_route with the two flags (host side, no device touched) */
int32_t iisan_gemm16_h256_applicable_blk32(int32_t mode, int64_t M, int32_t N, int32_t K, int32_t qkv_S, int32_t with_rowstat,
                                           int32_t a_blk32, int32_t out_blk32);
int32_t iisan_gemm16_route_blk32(int32_t dtype16, int32_t mode, int64_t M, int32_t N, int32_t K, int32_t qkv_S, int32_t qkv_heads,
                                 int32_t qkv_which0, int32_t with_rowstat, int32_t a_blk32, int32_t out_blk32);

#ifdef __cplusplus
}
#endif
#endif /* IISAN_HIP_H */
