// The VoxelNet detection loss (section 2.2 of the paper; focal form with gamma > 0) on the (M,16) head against the
// 0 / 1 / 2 label code of lisec_rpn_labels (include/lisec_hip.h, lisec_detection_loss*): the three launches of
// detection_loss_parts.h.  The evaluation entry is the same three launches with a NULL gradient, so a sweep's values are
// the training entry's bits.
#include "detection_loss_parts.h"

namespace lisec {
namespace {

int run_det(const lisec_detection_loss_cfg& cfg, const float* head, const float* y_cls, const float* y_reg, long long M,
            float grad_scale, float* dhead, float* loss_out, long long* counts_out, double* acc, void* workspace,
            hipStream_t st, const lisec_sample_weights* sw = nullptr) {
    Carver ws(workspace);
    long long* counts = ws.take<long long>(2);
    double* parts = ws.take<double>((size_t)kDetBlocks * kDetVals);
    const int nb = grid_blocks(M * 16, kDetThreads, kDetBlocks);
    LISEC_LAUNCH(k_det_count, dim3(1), dim3(kCountThreads), 0, st, y_cls, M * 2, counts, counts_out);
    if (sw)
        LISEC_LAUNCH(k_det_loss<true, CellWeights>, dim3(nb), dim3(kDetThreads), 0, st, cfg, head, y_cls, y_reg, M, grad_scale,
                     counts, dhead, parts, cell_weights(*sw));
    else
        LISEC_LAUNCH(k_det_loss<false>, dim3(nb), dim3(kDetThreads), 0, st, cfg, head, y_cls, y_reg, M, grad_scale, counts, dhead,
                     parts);
    LISEC_LAUNCH(k_det_finalize, dim3(1), dim3(256), 0, st, cfg, parts, nb, counts, loss_out, acc);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" size_t lisec_detection_loss_workspace_bytes(void) {
    return align_up(2 * sizeof(long long), 256) + align_up(sizeof(double) * (size_t)kDetBlocks * kDetVals, 256);
}

extern "C" int lisec_detection_loss(const lisec_detection_loss_cfg* cfg, const float* head, const float* y_cls,
                                    const float* y_reg, long long M, float grad_scale, float* dhead, float* loss_out,
                                    long long* counts_out, void* workspace, size_t workspace_bytes, lisec_stream_t stream_) {
    if (int rc = check_det(cfg, M, workspace, workspace_bytes)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && dhead && loss_out && counts_out, "detection loss: NULL pointer");
    return run_det(*cfg, head, y_cls, y_reg, M, grad_scale, dhead, loss_out, counts_out, nullptr, workspace,
                   static_cast<hipStream_t>(stream_));
}

extern "C" int lisec_detection_loss_eval(const lisec_detection_loss_cfg* cfg, const float* head, const float* y_cls,
                                         const float* y_reg, long long M, double* acc, void* workspace,
                                         size_t workspace_bytes, lisec_stream_t stream_) {
    if (int rc = check_det(cfg, M, workspace, workspace_bytes)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && acc, "detection loss: NULL pointer");
    return run_det(*cfg, head, y_cls, y_reg, M, 1.0f, nullptr, nullptr, nullptr, acc, workspace,
                   static_cast<hipStream_t>(stream_));
}

// The weighted entries: the same three launches with the weighted k_det_loss in the middle, the same workspace.
extern "C" size_t lisec_detection_loss_weighted_workspace_bytes(void) { return lisec_detection_loss_workspace_bytes(); }

extern "C" int lisec_detection_loss_weighted(const lisec_detection_loss_cfg* cfg, const lisec_sample_weights* sw,
                                             const float* head, const float* y_cls, const float* y_reg, long long M,
                                             float grad_scale, float* dhead, float* loss_out, long long* counts_out,
                                             void* workspace, size_t workspace_bytes, lisec_stream_t stream_) {
    if (int rc = check_det(cfg, M, workspace, workspace_bytes)) return rc;
    if (int rc = check_sample_weights(sw, nullptr)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && dhead && loss_out && counts_out, "detection loss: NULL pointer");
    return run_det(*cfg, head, y_cls, y_reg, M, grad_scale, dhead, loss_out, counts_out, nullptr, workspace,
                   static_cast<hipStream_t>(stream_), sw);
}

extern "C" int lisec_detection_loss_weighted_eval(const lisec_detection_loss_cfg* cfg, const lisec_sample_weights* sw,
                                                  const float* head, const float* y_cls, const float* y_reg, long long M,
                                                  double* acc, void* workspace, size_t workspace_bytes,
                                                  lisec_stream_t stream_) {
    if (int rc = check_det(cfg, M, workspace, workspace_bytes)) return rc;
    if (int rc = check_sample_weights(sw, nullptr)) return rc;
    LISEC_CHECK_ARG(head && y_cls && y_reg && acc, "detection loss: NULL pointer");
    return run_det(*cfg, head, y_cls, y_reg, M, 1.0f, nullptr, nullptr, nullptr, acc, workspace,
                   static_cast<hipStream_t>(stream_), sw);
}
