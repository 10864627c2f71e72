// csrc/loss_plan.h alone, as a host program (tests/test_soft_f_loss_host.py builds it with ASan + UBSan): every refusal of soft_f_validate in
// the order of its codes, the limits on both sides, and the launch constants.  Prints "FAILED ..." per broken invariant and ends with
// "ok: 0 failed checks".
#include <stdio.h>
#include <initializer_list>
#include <limits>
#include "../../multi-modal-emotion_amd/csrc/loss_plan.h"
#include "check.h"

using namespace tav::plan;

int main() {
    static float buf[64];
    static int64_t tgt[4];
    tav_soft_f_args a = {};
    CHECK(soft_f_validate(nullptr) == TAV_ERR_NULL && soft_f_validate(&a) == TAV_ERR_NULL, "null");
    a.logits = buf; a.target = tgt; a.loss = buf; a.dlogits = buf;
    a.B = 4; a.C = 7; a.ld = 7; a.beta = 0.5; a.eps = 1e-7; a.grad_scale = 1.f; a.mode = TAV_SOFT_F_FBETA;
    CHECK(soft_f_validate(&a) == 0, "plain: %d", soft_f_validate(&a));
    tav_soft_f_args b = a;
    b.logits = nullptr;                          CHECK(soft_f_validate(&b) == TAV_ERR_NULL, "logits");
    b = a; b.target = nullptr;                   CHECK(soft_f_validate(&b) == TAV_ERR_NULL, "target");
    b = a; b.loss = nullptr;                     CHECK(soft_f_validate(&b) == 0, "gradient only");
    b = a; b.dlogits = nullptr;                  CHECK(soft_f_validate(&b) == 0, "loss only");
    b = a; b.loss = nullptr; b.dlogits = nullptr; b.stats = buf;    CHECK(soft_f_validate(&b) == TAV_ERR_NULL, "no output");
    b = a; b.weight = buf; b.stats = buf;        CHECK(soft_f_validate(&b) == 0, "optional pointers");
    long accepted = 0, refused = 0;
    for (int64_t B : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)TAV_SOFT_F_MAX_B, (int64_t)TAV_SOFT_F_MAX_B + 1})
        for (int64_t C = -1; C <= TAV_SOFT_F_MAX_C + 1; ++C)
            for (int64_t ld : {C - 1, C, C + 3, SOFT_F_MAX_LD, SOFT_F_MAX_LD + 1}) {
                b = a; b.B = B; b.C = C; b.ld = ld;
                const bool ok = B >= 1 && B <= TAV_SOFT_F_MAX_B && C >= 1 && C <= TAV_SOFT_F_MAX_C && ld >= C && ld <= SOFT_F_MAX_LD;
                CHECK(soft_f_validate(&b) == (ok ? 0 : TAV_ERR_SHAPE), "B %ld C %ld ld %ld: %d", (long)B, (long)C, (long)ld, soft_f_validate(&b));
                ++(ok ? accepted : refused);
            }
    CHECK(accepted > 0 && refused > 0, "%ld accepted, %ld refused", accepted, refused);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double v : {0.0, -1.0, inf, -inf, nan}) {
        b = a; b.beta = v;                       CHECK(soft_f_validate(&b) == TAV_ERR_SHAPE, "beta %g", v);
        b = a; b.eps = v;                        CHECK(soft_f_validate(&b) == TAV_ERR_SHAPE, "eps %g", v);
    }
    b = a; b.eps = 0.5;                          CHECK(soft_f_validate(&b) == TAV_ERR_SHAPE, "eps 0.5");
    b = a; b.eps = 0.25; b.beta = 1e30;          CHECK(soft_f_validate(&b) == 0, "large finite scalars");
    for (int mode : {-1, 2, 7}) { b = a; b.mode = mode; CHECK(soft_f_validate(&b) == TAV_ERR_SHAPE, "mode %d", mode); }
    b = a; b.mode = TAV_SOFT_F_PRECISION;        CHECK(soft_f_validate(&b) == 0, "precision");
    b = a; b.B = 0; b.logits = nullptr;          CHECK(soft_f_validate(&b) == TAV_ERR_NULL, "pointers before sizes");
    b = a; b.B = 0; b.beta = nan;                CHECK(soft_f_validate(&b) == TAV_ERR_SHAPE, "sizes");
    CHECK(SOFT_F_BLOCK == 64 * SOFT_F_WAVES && SOFT_F_BLOCK >= TAV_SOFT_F_MAX_C && LOSS_ABI_VERSION == 1, "launch constants");
    printf("accepted %ld refused %ld\n", accepted, refused);
    return check_summary();
}
