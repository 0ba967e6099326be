// The two statements that turn UNetLoss's cross entropy into the focal and the soft Dice loss, each stated once:
// loss.hip's kernels call them per pixel / per (document, class), and with -DMSAU_COST_CPU this header alone compiles as plain C++
// (tests/test_unet_cost_cpu.py builds it with the host compiler and checks the edge cases without a GPU).  fp32, plain operations,
// powf of the math library: no fast-math form.
#pragma once
#include <math.h>

#ifdef MSAU_COST_CPU
#define MSAU_COST_FN static inline
#else
#define MSAU_COST_FN __host__ __device__ __forceinline__
#endif

// Focal loss of Lin et al. at one pixel.  pt = softmax[label], nll = -log(pt) as the CE kernels have them, gamma >= 0.
//   *f = (1 - pt)^gamma                                        : the pixel's loss is f * nll
//   *m = f + gamma * pt * (1 - pt)^(gamma - 1) * nll           : its gradient is m * (softmax - onehot)
// gamma == 0 is the cross entropy: f = m = 1 exactly, whatever pt.  Where 1 - pt rounds to 0 (and gamma > 0) the pixel has
// f = m = 0: the plain form would multiply 0^(gamma - 1) = inf by 0.
MSAU_COST_FN void msau_focal_factor(float pt, float nll, float gamma, float* f, float* m) {
    const float q = 1.f - pt;
    if (gamma == 0.f) { *f = 1.f; *m = 1.f; return; }
    if (!(q > 0.f)) { *f = 0.f; *m = 0.f; return; }
    const float qg = powf(q, gamma);
    *f = qg;
    *m = qg + gamma * pt * (qg / q) * nll;
}

// Soft Dice of one class of one document.  I = sum p_c [y = c], P = sum p_c, Y = sum [y = c] over the document's active pixels,
// eps > 0, vn = v_c / V (0 when V = sum_c v_c is 0).
//   *term = vn * dice_c,  dice_c = (2 I + eps) / (P + Y + eps)  : the document's loss is 1 - sum_c term (msau_dice_loss)
//   *miss = vn * (2 I + eps) / den^2,  *hit = miss - vn * 2 / den  : dL/dx_j = p_j (a_j - sum_c a_c p_c), a_c = hit at c = y else miss
MSAU_COST_FN void msau_dice_coef(float I, float P, float Y, float eps, float vn, float* term, float* hit, float* miss) {
    const float den = P + Y + eps, num = 2.f * I + eps;
    *term = vn * (num / den);
    *miss = vn * num / (den * den);
    *hit = *miss - vn * 2.f / den;
}
// the document's loss from V = sum_c v_c and s = sum_c term: 0 for a document without weight
MSAU_COST_FN float msau_dice_loss(float V, float s) { return V > 0.f ? 1.f - s : 0.f; }

#ifdef MSAU_COST_CPU
extern "C" void msau_focal_factor_cpu(float pt, float nll, float gamma, float* f, float* m) { msau_focal_factor(pt, nll, gamma, f, m); }
extern "C" void msau_dice_coef_cpu(float I, float P, float Y, float eps, float vn, float* term, float* hit, float* miss) {
    msau_dice_coef(I, P, Y, eps, vn, term, hit, miss);
}
extern "C" float msau_dice_loss_cpu(float V, float s) { return msau_dice_loss(V, s); }
#endif
