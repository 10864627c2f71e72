/* libtavhip, soft F-score losses -- package-private entry points of libtavhip.so (bound by _lib.PRIVATE_ABIS, not installed under include/).
 *
 * The reference's second sweep of the tri-modal model trains with FBetaLoss / PrecisionLoss (TripleModels/tav_nn.py:92-98); the
 * definition that survives is the soft F1 of notebooks/loss.ipynb.  tav_soft_f_loss is that family with beta = 1 equal to the notebook's
 * function.  It follows the rules of include/tavhip.h (extern "C", device pointers and sizes, `stream` a hipStream_t passed as void*, no
 * allocation, no synchronisation, TAV_ERR_* codes) and lives in the same shared object.  The header stays next to the sources because
 * the symbol sets and versions of the headers under include/ are pinned by recorded tables; a change that re-records those tables moves
 * this file to include/ as the fifth public header (and gives it the C guard of the others: until then it is read by C++ only, and
 * csrc/ carries no conditional compilation).  tav_loss_version() is bumped on any signature change.
 */
#ifndef TAVHIP_LOSS_H
#define TAVHIP_LOSS_H
#include <stdint.h>
#include "../../include/tavhip.h"

extern "C" {

int tav_loss_version(void);

#define TAV_SOFT_F_FBETA 0
#define TAV_SOFT_F_PRECISION 1
#define TAV_SOFT_F_MAX_B 65536
#define TAV_SOFT_F_MAX_C 16

/* With p_b = softmax(z_b) in f32 (max subtracted), over the B rows of the batch and the C classes:
 *     tp_k = sum_b [t_b = k] p_bk     fp_k = sum_b [t_b != k] p_bk     fn_k = sum_b [t_b = k] (1 - p_bk)          (f64 sums, fixed order)
 *     P_k = tp_k / (tp_k + fp_k + eps)                R_k = tp_k / (tp_k + fn_k + eps)
 *     F_k = (1 + beta^2) P_k R_k / (beta^2 P_k + R_k + eps)   (TAV_SOFT_F_FBETA)       F_k = P_k   (TAV_SOFT_F_PRECISION)
 *     loss = 1 - sum_k w_k clamp(F_k, eps, 1 - eps)                                    (f64, rounded to f32 at the store)
 *     dlogits_bk = grad_scale p_bk (g_bk - sum_j p_bj g_bj),   g_bk = [t_b = k] (dloss/dtp_k - dloss/dfn_k) + [t_b != k] dloss/dfp_k
 * The clamp passes the gradient where eps <= F_k <= 1 - eps and stops it outside (torch.clamp).  A target outside [0, C) belongs to no
 * class: its row counts towards every fp_k.  One launch of one workgroup writes loss and dlogits; the bits do not depend on the run.
 * 1 <= B <= TAV_SOFT_F_MAX_B, 1 <= C <= TAV_SOFT_F_MAX_C, C <= ld <= 2^40; beta and eps finite and > 0, eps < 0.5. */
typedef struct tav_soft_f_args {
    const float* logits;        /* [B] rows of C logits, row stride ld elements                      */
    const int64_t* target;      /* [B]                                                               */
    const float* weight;        /* optional [C]; NULL: every w_k = 1                                 */
    float* loss;                /* optional [1]; at least one of loss and dlogits                    */
    float* dlogits;             /* optional [B][C] dense                                             */
    float* stats;               /* optional [3][C]: tp, fp, fn as the class stage saw them           */
    int64_t B, C, ld;
    double beta, eps;
    float grad_scale;
    int32_t mode;               /* TAV_SOFT_F_FBETA or TAV_SOFT_F_PRECISION                          */
} tav_soft_f_args;
int tav_soft_f_loss(const tav_soft_f_args* args, void* stream);

}
#endif
