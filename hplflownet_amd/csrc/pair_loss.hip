// pair_loss.hip -- the loss op of a training step whose per-pair losses and gradients somebody else computed (include/hpl_bcl.h
// "Pair losses"): hpl_pair_grad hands hpl_selfsup_loss's dL_b / dflow to the backward as the gradient of the
// mean over the batch's pairs -- every row times 1 / batch -- and leaves the batch loss as the ascending float32 fold of the
// per-pair losses, from a second launch of one wave: no atomic, no workgroup that waits for another.
#include "cloud_common.h"

using namespace hpl;

namespace {

// One wave: lane b fetches pair b's loss, lane 0 adds them in ascending b from 0 and divides by the batch.
__global__ void __launch_bounds__(64) k_fold_pair_loss(const float *__restrict__ pair_loss, int stride, int batch,
                                                       float *__restrict__ loss) {
    __shared__ float v[CLOUD_MAX_BATCH];
    const int t = threadIdx.x;
    if (t < batch) v[t] = pair_loss[(int64_t)t * stride];
    __syncthreads();
    if (t != 0) return;
    float s = 0.f;
    for (int b = 0; b < batch; ++b) s += v[b];
    *loss = s / (float)batch;
}

// grad[i] = dflow[i] * w, i < total: `head` scalar elements up to the first 16-byte boundary (dflow and grad sit alike relative
// to one: the host checked), float4 words, a scalar tail.  head = total: every element scalar.
__global__ void __launch_bounds__(256) k_pair_grad(const float *__restrict__ dflow, float *__restrict__ grad, int64_t total,
                                                   int64_t head, float w) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int64_t n4 = (total - head) / 4;
    const float4 *s4 = reinterpret_cast<const float4 *>(dflow + head);
    float4 *d4 = reinterpret_cast<float4 *>(grad + head);
    for (int64_t i = tid; i < n4; i += stride) {
        float4 v = s4[i];
        v.x *= w; v.y *= w; v.z *= w; v.w *= w;
        d4[i] = v;
    }
    // the elements outside the words: [0, head) and [head + 4 n4, total), fewer than 4 + 4 unless everything is scalar
    const int64_t tail0 = head + 4 * n4, loose = head + (total - tail0);
    for (int64_t i = tid; i < loose; i += stride) {
        const int64_t e = i < head ? i : tail0 + (i - head);
        grad[e] = dflow[e] * w;
    }
}

int fold(const char *op, const float *pair_loss, int stride, int batch, float *loss, hipStream_t s) {
    if (!loss) return HPL_OK;
    k_fold_pair_loss<<<1, 64, 0, s>>>(pair_loss, stride, batch, loss);
    HPL_CHECK_LAUNCH(op);
    return HPL_OK;
}

}  // namespace

extern "C" int hpl_pair_grad(const float *dflow, int64_t rows, int batch, const float *pair_loss, int loss_stride, float *grad,
                             float *loss, hplStream stream) {
    const char *op = "hpl_pair_grad";
    HPL_CLOUD_CHECK(check_batch(op, batch));
    HPL_REQUIRE(grad || loss, "%s: neither a gradient nor a loss is asked for", op);
    HPL_REQUIRE(!grad || dflow, "%s: null dflow", op);
    HPL_REQUIRE(!loss || (pair_loss && loss_stride >= 1), "%s: the batch loss is the fold of pair_loss (null, or stride %d < 1)", op,
                loss_stride);
    HPL_REQUIRE(rows >= 0, "%s: %lld rows", op, (long long)rows);
    HPL_CLOUD_CHECK(check_points(op, rows));
    HPL_CLOUD_CHECK(check_aligned4(op, {dflow, pair_loss, grad, loss}));
    hipStream_t s = to_stream(stream);
    const int64_t total = rows * 3;
    if (grad && total > 0) {
        // 16-byte words where both arrays reach a boundary after the same number of elements
        const uintptr_t a = reinterpret_cast<uintptr_t>(dflow) & 15u, g = reinterpret_cast<uintptr_t>(grad) & 15u;
        const int64_t head = a == g ? imin((int64_t)((16 - a) & 15u) / 4, total) : total;
        const int64_t n4 = (total - head) / 4, work = imax(n4, total - 4 * n4);          // words, or the elements outside them
        k_pair_grad<<<(int)imin(cdiv(work, 256), 4096), 256, 0, s>>>(dflow, grad, total, head, 1.0f / (float)batch);
        HPL_CHECK_LAUNCH(op);
    }
    return fold(op, pair_loss, loss_stride, batch, loss, s);
}
