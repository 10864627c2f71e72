// Host decisions of the soft F-score loss (loss.hip, tavhip_loss.h) as pure functions: the argument checks and the launch shape of
// tav_soft_f_loss.  Only the headers and the standard library, no HIP type: any C++17 host compiler builds it
// (tests/host/loss_plan_check.cpp runs it under ASan + UBSan).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include "tavhip_loss.h"

namespace tav {
namespace plan {

constexpr int LOSS_ABI_VERSION = 1;
constexpr int SOFT_F_BLOCK = 256;                 // one workgroup of four waves: thread i takes rows i, i + 256, ...
constexpr int SOFT_F_WAVES = SOFT_F_BLOCK / 64;
constexpr int64_t SOFT_F_MAX_LD = (int64_t)1 << 40;

inline bool soft_f_positive(double v) { return isfinite(v) && v > 0.0; }
// the order of the tests is the order of the codes: pointers, then sizes, then the scalars
inline int soft_f_validate(const tav_soft_f_args* a) {
    if (!a || !a->logits || !a->target || (!a->loss && !a->dlogits)) return TAV_ERR_NULL;
    if (a->B < 1 || a->B > TAV_SOFT_F_MAX_B || a->C < 1 || a->C > TAV_SOFT_F_MAX_C) return TAV_ERR_SHAPE;
    if (a->ld < a->C || a->ld > SOFT_F_MAX_LD) return TAV_ERR_SHAPE;
    if (!soft_f_positive(a->beta) || !soft_f_positive(a->eps) || a->eps >= 0.5) return TAV_ERR_SHAPE;
    if (a->mode != TAV_SOFT_F_FBETA && a->mode != TAV_SOFT_F_PRECISION) return TAV_ERR_SHAPE;
    return 0;
}

}  // namespace plan
}  // namespace tav
