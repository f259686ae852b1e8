// User-side inputs built on the device (include/iisan_hip.h: "Device-resident user store"): the left-padded token windows, masks and
// targets of a user batch, its 0-padded exclusion lists, and the histogram of a rank vector.  The sequences live in CSR form (off int64
// [n_users + 1], items int32 [nnz]); a batch names its users by an int64 index on the device, so no per-batch tensor is built on the host.
//
// These are row gathers — no arithmetic, no LDS for the windows: one wave per window row, lane j owns column j of the row (S + 1 <= 64), and
// the optional embedding gather x[b, j] = item_emb[ids[b, j]] moves 16 bytes per lane, the column's id handed round the wave by a shuffle.
#include "common.h"

namespace {

constexpr int WIN_WAVES = 4;           // window rows per workgroup (one wave each)
constexpr int WIN_MAX_S = 63;          // the loss's limit (S + 1 columns of a TRAIN row fit one wave)
constexpr int HISTO_MAX_K = 64;

int64_t g_cnt_windows = 0, g_cnt_history = 0, g_cnt_histogram = 0;
IISAN_DEV_COUNTER(user_windows, g_cnt_windows);
IISAN_DEV_COUNTER(user_history, g_cnt_history);
IISAN_DEV_COUNTER(rank_histogram, g_cnt_histogram);

// MODE: IISAN_WIN_TRAIN / IISAN_WIN_EVAL / IISAN_WIN_INPUT.  W = columns of `ids` (S + 1 in TRAIN mode, else S); log_mask always has S.
template <int MODE>
__global__ __launch_bounds__(WIN_WAVES * WAVE) void user_windows_kernel(
    const int64_t* __restrict__ off, const int32_t* __restrict__ items, int64_t n_users, const int64_t* __restrict__ user_index, int64_t B,
    int S, int64_t* __restrict__ ids, float* __restrict__ log_mask, int32_t* __restrict__ target, const float* __restrict__ item_emb,
    int64_t n_items_plus1, int E, float* __restrict__ x) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t b = (int64_t)blockIdx.x * WIN_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;                                   // whole waves leave: the shuffles below see full waves
    const int W = MODE == IISAN_WIN_TRAIN ? S + 1 : S;
    const int64_t u = user_index[b];
    int64_t base = 0, L = 0;
    if (u >= 0 && u < n_users) {                          // anything else is a padding row: nothing of the store is read
        base = off[u];
        L = off[u + 1] - base;
        if (L < 0) L = 0;
    }
    // the window = the n items that end at position `end` of the sequence
    const int64_t end = MODE == IISAN_WIN_EVAL ? (L > 0 ? L - 1 : 0) : L;
    const int n = (int)(end < W ? end : W);
    const int k = lane - (W - n);                         // position inside the window; < 0: left padding
    int32_t id = 0;
    if (lane < W && k >= 0) id = items[base + end - n + k];
    if (lane < W) ids[b * W + lane] = id;
    if (lane < S) log_mask[b * S + lane] = k >= 0 ? 1.0f : 0.0f;
    if (target != nullptr && lane == 0) target[b] = (MODE == IISAN_WIN_EVAL && L > 0) ? items[base + L - 1] : 0;
    if constexpr (MODE != IISAN_WIN_TRAIN) {
        if (x == nullptr) return;
        const int per = E >> 2;                           // 16-byte pieces of a table row
        const int total = S * per;
        float* xr = x + b * (int64_t)S * E;
        for (int c0 = 0; c0 < total; c0 += WAVE) {        // uniform trip count: every lane takes part in the shuffle
            const int c = c0 + lane;
            const int j = c < total ? c / per : 0;
            const int32_t idj = __shfl(id, j, WAVE);
            if (c < total) {
                f4 v = {0.f, 0.f, 0.f, 0.f};
                if (idj >= 0 && idj < n_items_plus1) v = *(const f4*)(item_emb + (int64_t)idj * E + (c - j * per) * 4);
                *(f4*)(xr + (int64_t)c * 4) = v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void user_history_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ items, int64_t n_users,
                                                           const int64_t* __restrict__ user_index, int64_t B, int stride,
                                                           int32_t* __restrict__ history) {
    const int64_t total = B * stride;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / stride, k = i - b * stride;
        const int64_t u = user_index[b];
        int32_t v = 0;
        if (u >= 0 && u < n_users) {
            const int64_t base = off[u];
            if (k < off[u + 1] - base) v = items[base + k];
        }
        history[i] = v;
    }
}

// bins: 0 = ranks < 1, r = rank r (1 <= r <= K), K + 1 = ranks > K.  Integer adds only (LDS, then one 64-bit global add per non-empty bin
// and workgroup): the counts do not depend on the launch's schedule.
__global__ __launch_bounds__(256) void rank_histogram_kernel(const int32_t* __restrict__ ranks, int64_t U, int K,
                                                             unsigned long long* __restrict__ counts) {
    __shared__ unsigned int bins[HISTO_MAX_K + 2];
    for (int t = threadIdx.x; t < K + 2; t += blockDim.x) bins[t] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < U; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = ranks[i];
        atomicAdd(&bins[r < 1 ? 0 : (r > K ? K + 1 : r)], 1u);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < K + 2; t += blockDim.x)
        if (bins[t]) atomicAdd(&counts[t], (unsigned long long)bins[t]);
}

}  // namespace

extern "C" int iisan_user_windows(const int64_t* seq_off, const int32_t* seq_items, int64_t n_users, const int64_t* user_index, int64_t B,
                                  int32_t S, int32_t mode, int64_t* ids, float* log_mask, int32_t* target, const float* item_emb,
                                  int64_t n_items_plus1, int32_t E, float* x, void* stream) {
    IISAN_CHECK_SHAPE(mode == IISAN_WIN_TRAIN || mode == IISAN_WIN_EVAL || mode == IISAN_WIN_INPUT, "user_windows: unknown mode %d", mode);
    IISAN_CHECK_SHAPE(B > 0, "user_windows: B = %lld must be positive", (long long)B);
    IISAN_CHECK_SHAPE(B < (1ll << 31), "user_windows: B = %lld too large", (long long)B);
    IISAN_CHECK_SHAPE(S >= 1 && S <= WIN_MAX_S, "user_windows: S = %d outside 1..%d", S, WIN_MAX_S);
    IISAN_CHECK_SHAPE(n_users >= 0, "user_windows: n_users = %lld is negative", (long long)n_users);
    IISAN_CHECK_SHAPE(seq_off != nullptr, "user_windows: seq_off is null");
    IISAN_CHECK_SHAPE(seq_items != nullptr, "user_windows: seq_items is null");
    IISAN_CHECK_SHAPE(user_index != nullptr, "user_windows: user_index is null");
    IISAN_CHECK_SHAPE(ids != nullptr, "user_windows: ids is null");
    IISAN_CHECK_SHAPE(log_mask != nullptr, "user_windows: log_mask is null");
    IISAN_CHECK_SHAPE(mode != IISAN_WIN_EVAL || target != nullptr, "user_windows: target is null in EVAL mode");
    if (x != nullptr) {
        IISAN_CHECK_SHAPE(mode != IISAN_WIN_TRAIN, "user_windows: x is not produced in TRAIN mode");
        IISAN_CHECK_SHAPE(item_emb != nullptr, "user_windows: x given without item_emb");
        IISAN_CHECK_SHAPE(E > 0 && E % 4 == 0, "user_windows: E = %d must be a positive multiple of 4", E);
        IISAN_CHECK_SHAPE(n_items_plus1 > 0, "user_windows: n_items_plus1 = %lld must be positive", (long long)n_items_plus1);
        IISAN_CHECK_SHAPE(((uintptr_t)item_emb | (uintptr_t)x) % 16 == 0, "user_windows: item_emb and x must be 16-byte aligned");
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(B, WIN_WAVES)), block(WIN_WAVES * WAVE);
#define IISAN_WIN_LAUNCH(MODE)                                                                                                         \
    hipLaunchKernelGGL(user_windows_kernel<MODE>, grid, block, 0, s, seq_off, seq_items, n_users, user_index, B, (int)S, ids, log_mask, \
                       target, item_emb, n_items_plus1, (int)E, x)
    if (mode == IISAN_WIN_TRAIN) IISAN_WIN_LAUNCH(IISAN_WIN_TRAIN);
    else if (mode == IISAN_WIN_EVAL) IISAN_WIN_LAUNCH(IISAN_WIN_EVAL);
    else IISAN_WIN_LAUNCH(IISAN_WIN_INPUT);
#undef IISAN_WIN_LAUNCH
    ++g_cnt_windows;
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

extern "C" int iisan_user_history(const int64_t* hist_off, const int32_t* hist_items, int64_t n_users, const int64_t* user_index, int64_t B,
                                  int32_t hist_stride, int32_t* history, void* stream) {
    IISAN_CHECK_SHAPE(B > 0, "user_history: B = %lld must be positive", (long long)B);
    IISAN_CHECK_SHAPE(hist_stride >= 1, "user_history: hist_stride = %d must be at least 1", hist_stride);
    IISAN_CHECK_SHAPE(n_users >= 0, "user_history: n_users = %lld is negative", (long long)n_users);
    IISAN_CHECK_SHAPE(hist_off != nullptr, "user_history: hist_off is null");
    IISAN_CHECK_SHAPE(hist_items != nullptr, "user_history: hist_items is null");
    IISAN_CHECK_SHAPE(user_index != nullptr, "user_history: user_index is null");
    IISAN_CHECK_SHAPE(history != nullptr, "user_history: history is null");
    const int64_t blocks = ceil_div(B * hist_stride, 256);
    hipLaunchKernelGGL(user_history_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, hist_off,
                       hist_items, n_users, user_index, B, (int)hist_stride, history);
    ++g_cnt_history;
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

extern "C" int iisan_rank_histogram(const int32_t* ranks, int64_t U, int32_t K, int64_t* counts, void* stream) {
    IISAN_CHECK_SHAPE(U > 0, "rank_histogram: U = %lld must be positive", (long long)U);
    IISAN_CHECK_SHAPE(K >= 1 && K <= HISTO_MAX_K, "rank_histogram: K = %d outside 1..%d", K, HISTO_MAX_K);
    IISAN_CHECK_SHAPE(ranks != nullptr, "rank_histogram: ranks is null");
    IISAN_CHECK_SHAPE(counts != nullptr, "rank_histogram: counts is null");
    const int64_t blocks = ceil_div(U, 256 * 8);          // ~8 ranks per thread before the global adds
    hipLaunchKernelGGL(rank_histogram_kernel, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(256), 0, (hipStream_t)stream, ranks, U,
                       (int)K, (unsigned long long*)counts);
    ++g_cnt_histogram;
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}
