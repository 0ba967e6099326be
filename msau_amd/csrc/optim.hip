// The optimisers of the reference's get_optimizer (model/training/optimizer.py) on the flat fp32 buffers: RMSprop, SGD with
// momentum and Adam, each with weight decay, an optional global-norm clip and skip ranges (msau_optim_step).  A translation unit
// of its own: msau_clip_adam_step (elementwise.hip), which the default engine and the benchmark run, is not touched.
#include "msau_common.h"

namespace {

constexpr int kMaxBlocks = 512;          // the update's grid-stride grid (as adam_kernel's)
constexpr int kMaxSqBlocks = 128;        // partial sums of squares: two per lane of the wave that adds them up again

struct SkipRanges {
    int n;
    int64_t r[MSAU_OPTIM_MAX_SKIP][2];
};

int update_blocks(int64_t n) {
    const int64_t b = cdiv64(n, kThreads);
    return (int)(b < kMaxBlocks ? b : kMaxBlocks);
}
int sq_blocks(int64_t n) {
    const int b = update_blocks(n);
    return b < kMaxSqBlocks ? b : kMaxSqBlocks;
}

}  // namespace

// sum of squares of the gradient, one partial per workgroup in a fixed order (no atomics: the same bits on every run), and the
// step counter; under ADAM the bias corrections too, once, for every workgroup of the update
__global__ void optim_sqsum_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partials, float* __restrict__ state,
                                   int kind, double beta1, double beta2) {
    __shared__ float red[kThreads / 64];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        const float v0 = g[i], v1 = g[i + stride], v2 = g[i + 2 * stride], v3 = g[i + 3 * stride];
        s0 += v0 * v0; s1 += v1 * v1; s2 += v2 * v2; s3 += v3 * v3;
    }
    for (; i < n; i += stride) { const float v = g[i]; s0 += v * v; }
    float s = (s0 + s1) + (s2 + s3);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < kThreads / 64; ++w) t += red[w];
        partials[blockIdx.x] = t;
        if (blockIdx.x == 0) {
            const float step = state[0] + 1.f;
            state[0] = step;
            if (kind == MSAU_OPTIM_ADAM) {
                state[3] = (float)(1.0 - pow(beta1, (double)step));
                state[4] = (float)(1.0 - pow(beta2, (double)step));
            }
        }
    }
}

// NORM: the launch follows optim_sqsum_kernel; every workgroup derives the clip coefficient from the partials (fixed order: the
// same bits everywhere) and reads ADAM's bias corrections.  !NORM (RMSPROP / MOMENTUM without clipping): the only launch of the
// step; thread 0 of workgroup 0 bumps the step counter, which no thread of this launch reads.
// c1, c2: beta1, beta2 (ADAM); alpha, - (RMSPROP); momentum, - (MOMENTUM).  a, b: exp_avg, exp_avg_sq / square_avg, - / momentum_buffer, -.
// omc1, omc2: 1 - c1, 1 - c2 taken in double and rounded once, as torch hands them to its kernels (1.f - 0.999f is off by 5e-5).
template <int KIND, bool NORM>
__global__ void optim_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ a, float* __restrict__ b,
                                    float* __restrict__ state, const float* __restrict__ partials, int npart, int64_t n, float lr,
                                    float c1, float omc1, float c2, float omc2, float eps, float weight_decay, float max_norm,
                                    float grad_scale, SkipRanges skip) {
    __shared__ float sh[4];
    float coef = 1.f, bc1 = 1.f, bc2s = 1.f;
    if (NORM) {
        if (threadIdx.x < 64) {
            float s = 0.f;
            for (int i = threadIdx.x; i < npart; i += 64) s += partials[i];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
            if (threadIdx.x == 0) {
                const float norm = sqrtf(s) * grad_scale;
                float cf = 1.f;
                if (max_norm > 0.f) {
                    cf = max_norm / (norm + 1e-6f);                         // torch.nn.utils.clip_grad_norm_
                    cf = cf < 1.f ? cf : 1.f;
                }
                sh[0] = cf;
                if (KIND == MSAU_OPTIM_ADAM) { sh[1] = state[3]; sh[2] = state[4]; }
                if (blockIdx.x == 0) { state[1] = norm; state[2] = cf; }
            }
        }
        __syncthreads();
        coef = sh[0];
        if (KIND == MSAU_OPTIM_ADAM) { bc1 = sh[1]; bc2s = sqrtf(sh[2]); }
    } else if (blockIdx.x == 0 && threadIdx.x == 0) {
        state[0] = state[0] + 1.f;
    }
    const float step_size = lr / bc1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        bool skipped = false;
        for (int r = 0; r < skip.n; ++r) skipped |= (i >= skip.r[r][0]) & (i < skip.r[r][1]);
        if (skipped) continue;                               // a parameter without a gradient: torch leaves it and its state alone
        const float pi = p[i];
        const float gi = g[i] * grad_scale * coef + weight_decay * pi;
        if (KIND == MSAU_OPTIM_RMSPROP) {
            const float si = c1 * a[i] + omc1 * gi * gi;
            a[i] = si;
            p[i] = pi - lr * (gi / (sqrtf(si) + eps));
        } else if (KIND == MSAU_OPTIM_MOMENTUM) {
            const float bi = c1 * a[i] + gi;
            a[i] = bi;
            p[i] = pi - lr * bi;
        } else {
            const float mi = c1 * a[i] + omc1 * gi;
            const float vi = c2 * b[i] + omc2 * gi * gi;
            a[i] = mi; b[i] = vi;
            const float denom = sqrtf(vi) / bc2s + eps;
            p[i] = pi - step_size * (mi / denom);
        }
    }
}

extern "C" int64_t msau_optim_ws_floats(int64_t n) { return n > 0 ? sq_blocks(n) : 0; }

extern "C" int msau_optim_step(void* stream, int kind, float* params, const float* grads, float* state_a, float* state_b, float* state,
                               float* ws, int64_t n, float lr, double c1, double c2, float eps, float weight_decay, float max_norm,
                               float grad_scale, const int64_t* skip, int n_skip) {
    MSAU_CHECK_ARG(kind == MSAU_OPTIM_ADAM || kind == MSAU_OPTIM_RMSPROP || kind == MSAU_OPTIM_MOMENTUM, "optim_step: unknown kind %d", kind);
    MSAU_CHECK_ARG(params && grads && state_a && state && n > 0, "optim_step: null buffer or n <= 0");
    MSAU_CHECK_ARG(kind != MSAU_OPTIM_ADAM || state_b, "optim_step: ADAM needs state_b (exp_avg_sq)");
    const bool norm = kind == MSAU_OPTIM_ADAM || max_norm > 0.f;
    MSAU_CHECK_ARG(!norm || ws, "optim_step: the sum-of-squares pass needs the workspace (msau_optim_ws_floats)");
    MSAU_CHECK_ARG(n_skip >= 0 && n_skip <= MSAU_OPTIM_MAX_SKIP && (n_skip == 0 || skip), "optim_step: %d skip ranges (0 .. %d, not NULL)",
                   n_skip, MSAU_OPTIM_MAX_SKIP);
    SkipRanges sk;
    sk.n = n_skip;
    for (int r = 0; r < MSAU_OPTIM_MAX_SKIP; ++r) {
        sk.r[r][0] = r < n_skip ? skip[2 * r] : 0;
        sk.r[r][1] = r < n_skip ? skip[2 * r + 1] : 0;
        if (r >= n_skip) continue;
        MSAU_CHECK_ARG(sk.r[r][0] >= 0 && sk.r[r][0] < sk.r[r][1], "optim_step: skip range %d is [%lld, %lld): empty or reversed", r,
                       (long long)sk.r[r][0], (long long)sk.r[r][1]);
        MSAU_CHECK_ARG(sk.r[r][1] <= n, "optim_step: skip range %d ends at %lld, beyond n = %lld", r, (long long)sk.r[r][1], (long long)n);
        MSAU_CHECK_ARG(r == 0 || sk.r[r][0] >= sk.r[r - 1][1], "optim_step: skip range %d overlaps range %d or is not in ascending order", r, r - 1);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = update_blocks(n), nsq = sq_blocks(n);
    if (norm) {
        hipLaunchKernelGGL(optim_sqsum_kernel, dim3(nsq), dim3(kThreads), 0, s, grads, n, ws, state, kind, c1, c2);
        MSAU_CHECK_LAUNCH("optim_sqsum");
    }
#define MSAU_OPTIM_LAUNCH(KIND, NORM)                                                                                                  \
    hipLaunchKernelGGL((optim_update_kernel<KIND, NORM>), dim3(nb), dim3(kThreads), 0, s, params, grads, state_a, state_b, state, ws, nsq, \
                       n, lr, (float)c1, (float)(1.0 - c1), (float)c2, (float)(1.0 - c2), eps, weight_decay, max_norm, grad_scale, sk)
    if (kind == MSAU_OPTIM_ADAM) MSAU_OPTIM_LAUNCH(MSAU_OPTIM_ADAM, true);
    else if (kind == MSAU_OPTIM_RMSPROP) { if (norm) MSAU_OPTIM_LAUNCH(MSAU_OPTIM_RMSPROP, true); else MSAU_OPTIM_LAUNCH(MSAU_OPTIM_RMSPROP, false); }
    else { if (norm) MSAU_OPTIM_LAUNCH(MSAU_OPTIM_MOMENTUM, true); else MSAU_OPTIM_LAUNCH(MSAU_OPTIM_MOMENTUM, false); }
#undef MSAU_OPTIM_LAUNCH
    MSAU_CHECK_LAUNCH("optim_update");
    return 0;
}
