// metrics.hip -- the evaluation metrics of a batch of pairs in one launch (hpl_flow_metrics).
//
// The reference reports EPE3D / ACC3DS / ACC3DR / Outliers3D (evaluation_utils.py:4-19) and EPE2D / ACC2D of the flow projected
// into the camera (utils/geometry.py:42-65, evaluation_utils.py:22-36), in float32 numpy.  Per point this kernel restates that
// arithmetic operation by operation in fp32: the same expression order, IEEE division and square root (the build compiles with
// -ffp-contract=off and without fast-math, so `/` and sqrtf are correctly rounded and nothing is fused), thresholds compared as
// fp32 values.  The per-pair reductions are what may differ from numpy's float32 pairwise means: error sums in fp64, predicate
// counts as integers, both in a fixed order (one workgroup per pair, thread t sums points t, t + T, ... ascending, then a fixed
// tree) -- a pair's eight words are the same bits wherever it sits in a batch and however many pairs run with it.
#include "common.h"

namespace {

constexpr int MT = 1024;          // threads per pair
constexpr int MAX_PAIRS = 64;

__global__ void __launch_bounds__(MT) k_flow_metrics(const hpl_metrics_pair *__restrict__ pairs, double *__restrict__ out) {
    __shared__ double se3[MT], se2[MT];
    __shared__ uint32_t cnt[4][MT];
    const hpl_metrics_pair d = pairs[blockIdx.x];
    const int t = threadIdx.x;
    double e3 = 0.0, e2 = 0.0;
    uint32_t s3 = 0, r3 = 0, o3 = 0, a2 = 0;
    const bool cam = d.has_camera != 0;
    const float f = d.camera[0], cx = d.camera[1], cy = d.camera[2];
    const float kx = d.camera[3], ky = d.camera[4], kz = d.camera[5];
    for (int64_t p = t; p < d.n; p += MT) {
        const float q0 = d.pred[p * d.pred_sp], q1 = d.pred[d.pred_sc + p * d.pred_sp], q2 = d.pred[2 * d.pred_sc + p * d.pred_sp];
        const float g0 = d.gt[p * d.gt_sp], g1 = d.gt[d.gt_sc + p * d.gt_sp], g2 = d.gt[2 * d.gt_sc + p * d.gt_sp];
        // evaluate_3d: l2 = ||gt - pred||, relative = l2 / (||gt|| + 1e-4)
        const float d0 = g0 - q0, d1 = g1 - q1, d2 = g2 - q2;
        const float err = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
        const float rel = err / (sqrtf((g0 * g0 + g1 * g1) + g2 * g2) + 1e-4f);
        e3 += (double)err;
        s3 += (err < 0.05f) | (rel < 0.05f);
        r3 += (err < 0.1f) | (rel < 0.1f);
        o3 += (err > 0.3f) | (rel > 0.1f);
        if (cam) {
            const float x = d.pc1[p * d.pc1_sp], y = d.pc1[d.pc1_sc + p * d.pc1_sp], z = d.pc1[2 * d.pc1_sc + p * d.pc1_sp];
            // project_3d_to_2d of pc1, pc1 + gt (the reference's pc2) and pc1 + pred (its predicted_pc2)
            const float gx = x + g0, gy = y + g1, gz = z + g2;
            const float px = x + q0, py = y + q1, pz = z + q2;
            const float u1 = ((x * f + cx * z) + kx) / (z + kz), v1 = ((y * f + cy * z) + ky) / (z + kz);
            const float ug = ((gx * f + cx * gz) + kx) / (gz + kz), vg = ((gy * f + cy * gz) + ky) / (gz + kz);
            const float up = ((px * f + cx * pz) + kx) / (pz + kz), vp = ((py * f + cy * pz) + ky) / (pz + kz);
            // get_batch_2d_flow: flow = px2 - px1 for both; evaluate_2d on flow_gt - flow_pred, relative to ||flow_gt|| + 1e-5
            const float fxg = ug - u1, fyg = vg - v1, fxp = up - u1, fyp = vp - v1;
            const float ex = fxg - fxp, ey = fyg - fyp;
            const float epe = sqrtf(ex * ex + ey * ey);
            const float rel2 = epe / (sqrtf(fxg * fxg + fyg * fyg) + 1e-5f);
            e2 += (double)epe;
            a2 += (epe < 3.0f) | (rel2 < 0.05f);
        }
    }
    se3[t] = e3;
    se2[t] = e2;
    cnt[0][t] = s3;
    cnt[1][t] = r3;
    cnt[2][t] = o3;
    cnt[3][t] = a2;
    __syncthreads();
    for (int w = MT / 2; w > 0; w >>= 1) {
        if (t < w) {
            se3[t] += se3[t + w];
            se2[t] += se2[t + w];
#pragma unroll
            for (int k = 0; k < 4; ++k) cnt[k][t] += cnt[k][t + w];
        }
        __syncthreads();
    }
    double *o = out + (int64_t)blockIdx.x * 8;
    if (t == 0) {
        o[0] = (double)d.n;
        o[1] = se3[0];
        o[2] = (double)cnt[0][0];
        o[3] = (double)cnt[1][0];
        o[4] = (double)cnt[2][0];
        o[7] = 0.0;
        if (cam) {
            o[5] = se2[0];
            o[6] = (double)cnt[3][0];
        }
    }
}

}  // namespace

extern "C" int hpl_flow_metrics(const hpl_metrics_pair *pairs, int batch, hpl_metrics_pair *stage, double *out, hplStream stream) {
    HPL_REQUIRE(pairs && stage && out, "hpl_flow_metrics: null argument");
    HPL_REQUIRE(batch >= 1 && batch <= MAX_PAIRS, "hpl_flow_metrics: %d pairs (1 .. %d)", batch, MAX_PAIRS);
    for (int b = 0; b < batch; ++b) {
        const hpl_metrics_pair &d = pairs[b];
        HPL_REQUIRE(d.pred && d.gt && d.pc1, "hpl_flow_metrics: pair %d has a null pointer", b);
        HPL_REQUIRE(d.n >= 1 && d.n < INT32_MAX, "hpl_flow_metrics: pair %d has %lld points (1 .. 2^31 - 2)", b, (long long)d.n);
        HPL_REQUIRE(d.pred_sc >= 0 && d.pred_sp >= 0 && d.gt_sc >= 0 && d.gt_sp >= 0 && d.pc1_sc >= 0 && d.pc1_sp >= 0,
                    "hpl_flow_metrics: pair %d has a negative stride", b);
    }
    hipStream_t s = hpl::to_stream(stream);
    if (hipMemcpyAsync(stage, pairs, sizeof(hpl_metrics_pair) * batch, hipMemcpyHostToDevice, s) != hipSuccess) {
        hpl::set_error("hpl_flow_metrics: descriptor copy failed: %s", hipGetErrorString(hipGetLastError()));
        return HPL_EHIP;
    }
    k_flow_metrics<<<batch, MT, 0, s>>>(stage, out);
    HPL_CHECK_LAUNCH("hpl_flow_metrics");
    return HPL_OK;
}
