// Everything that reads logits against labels or turns logits into probabilities: label counts and histograms, the masked cross
// entropy and its two-head form, the weighted CE, UNetLoss for training and per-document evaluation, the confusion counts and the
// two softmax heads.  Every loss is one kernel; how it holds a pixel's logits -- in registers or re-read from the cache -- is the type
// Pixel<T, CS8> below, the only place where the two forms differ.  The CE and the Dice gradient, the label / extent / weight rules and
// the workgroup sum are each stated once and used by every kernel of the family: that, not a comment, is what makes the register and
// the cache form (and the training and the evaluation kernels) agree bit for bit.  Accumulation in fp32, every summation order fixed.
#include "msau_common.h"
#include "loss_cost.h"

namespace {

// =============================================================================================
// the family's shared statements
// =============================================================================================
// strictly greater: the first maximum wins; a NaN counts as the maximum, as in torch.argmax
__device__ __forceinline__ void first_max(float v, int c, float& bv, int& best) {
    if (v > bv || (v != v && bv == bv)) { bv = v; best = c; }
}

// How a pixel's logits are held is a type, Pixel<T, CS8>; every kernel below is written once against it.  The type has no members:
// what a thread holds of a pixel is a `Pixel::Held h` of the kernel's own, and the operations are static --
//   load(h, px, Cs, C, lab, xl)   the pixel's Cs stored values at px -> the log-sum-exp over the C real classes: max, then the __expf
//                              sum in channel order, mx + __logf(se); the register form leaves x[lab] in xl (0 when lab is no channel)
//   label_logit(h, lab, active, xl)   the logit at the label: the register form hands back load's xl; the cache form READS l[lab]
//                              wherever `active` is set (0 elsewhere), so lab must be a channel there.  A separate operation so that a
//                              kernel can state `active` after the load, where it is used: computed before it, the large register
//                              instances of unet_ce_kernel came out with other code
//   channels(C), logit(h, c)   a visit of the real channels in channel order is `for (c = 0; c < channels(C); ++c) if (c < C) ... logit(h, c)`
//                              under `#pragma unroll kUnroll`: the register form visits all Cs with every index a constant, the cache form
//                              loops over C
//   prob(h, c, lse)            the probability of real channel c, __expf(logit - lse)
//   store(h, dst, C, active, g)   all Cs stored channels of a gradient: g(c) in the real channels of an active pixel, exact zeros in the
//                              padded channels and everywhere on an inactive pixel
//   store_dot(h, dst, lse, C, active, a, g)   the same with s = sum_c a_c * prob(c) taken first, by fmaf in channel order: g(p_c, a_c, s);
//                              a_c = a(c, real), which reads memory only where `real` (a real channel of an active pixel) and is 0 elsewhere
// Why it is written this way and not as an object with a callback per visit (profiles/loss_forms.md): the register form's Held is a
// plain array and the visiting loop stands in the kernel, which is the shape the compiler saw before there was a type; an array
// inside a struct, a member function around load, or the first maximum's running pair local to a callee each changed the code of
// large instances.
// Register form (CS8 > 0): the Cs = 8 * CS8 stored values sit in x[], every index a compile-time constant so that the array stays in
// registers; 16-byte loads and stores; the padded channels add + 0.f onto a positive sum (and fmaf(0, 0, s) onto s); store_dot turns
// x[] into the probabilities once and keeps the a(c).
template <typename T, int CS8>
struct Pixel {
    static constexpr int kCs = CS8 * 8;
    static constexpr int kUnroll = kCs;
    static constexpr int kDiceChunk = kCs;                           // the Dice sums take every class in one sweep of the slab
    typedef float Held[kCs];
    static __device__ __forceinline__ int dice_sweeps(int) { return 1; }
    static __device__ __forceinline__ float load(Held& x, const T* __restrict__ px, int, int C, int lab, float& xl) {
        float mx = -INFINITY;
        xl = 0.f;
#pragma unroll
        for (int c0 = 0; c0 < kCs; c0 += 8) {
            typename Vec8<T>::type v = load8<T>(px + c0);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                x[c0 + jj] = (float)v[jj];
                if (c0 + jj < C) mx = fmaxf(mx, x[c0 + jj]);
                xl = (c0 + jj == lab) ? x[c0 + jj] : xl;
            }
        }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < kCs; ++c) se += c < C ? __expf(x[c] - mx) : 0.f;
        return mx + __logf(se);
    }
    static __device__ __forceinline__ float label_logit(const Held&, int, bool, float xl) { return xl; }
    static __device__ __forceinline__ int channels(int) { return kCs; }
    static __device__ __forceinline__ float logit(const Held& x, int c) { return x[c]; }
    static __device__ __forceinline__ float prob(const Held& x, int c, float lse) { return __expf(x[c] - lse); }
    template <typename G>
    static __device__ __forceinline__ void store(const Held&, T* __restrict__ dst, int C, bool active, G g) {
#pragma unroll
        for (int c0 = 0; c0 < kCs; c0 += 8) {
            typename Vec8<T>::type o;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                float v = 0.f;
                if (active && c0 + jj < C) v = g(c0 + jj);
                o[jj] = (T)v;
            }
            store8<T>(dst + c0, o);
        }
    }
    template <typename A, typename G>
    static __device__ __forceinline__ void store_dot(Held& x, T* __restrict__ dst, float lse, int C, bool active, A a, G g) {
        float ac[kCs];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < kCs; ++c) {
            const bool real = active && c < C;
            ac[c] = a(c, real);
            x[c] = real ? prob(x, c, lse) : 0.f;
            s = fmaf(ac[c], x[c], s);
        }
        store(x, dst, C, active, [&](int c) { return g(x[c], ac[c], s); });
    }
};

// Cache form (CS8 = 0; any class count): nothing is kept, the pixel's logits are read again through l[c] wherever they are used.
template <typename T>
struct Pixel<T, 0> {
    static constexpr int kCs = 0;                                    // the stored channel count is the kernel's run-time Cs
    static constexpr int kUnroll = 1;
    static constexpr int kDiceChunk = 32;                            // classes a thread sums per sweep of its slab
    struct Held { const T* __restrict__ l; int Cs; };
    static __device__ __forceinline__ int dice_sweeps(int C) { return (C + kDiceChunk - 1) / kDiceChunk; }
    static __device__ __forceinline__ float load(Held& h, const T* __restrict__ l, int Cs, int C, int, float& xl) {
        h.l = l;
        h.Cs = Cs;
        float mx = -INFINITY;
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, (float)l[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += __expf((float)l[c] - mx);
        xl = 0.f;
        return mx + __logf(se);
    }
    static __device__ __forceinline__ float label_logit(const Held& h, int lab, bool active, float) { return active ? (float)h.l[lab] : 0.f; }
    static __device__ __forceinline__ int channels(int C) { return C; }
    static __device__ __forceinline__ float logit(const Held& h, int c) { return (float)h.l[c]; }
    static __device__ __forceinline__ float prob(const Held& h, int c, float lse) { return __expf((float)h.l[c] - lse); }
    template <typename G>
    static __device__ __forceinline__ void store(const Held& h, T* __restrict__ dst, int C, bool active, G g) {
        for (int c = 0; c < h.Cs; ++c) {
            float v = 0.f;
            if (active && c < C) v = g(c);
            dst[c] = (T)v;
        }
    }
    template <typename A, typename G>
    static __device__ __forceinline__ void store_dot(Held& h, T* __restrict__ dst, float lse, int C, bool active, A a, G g) {
        float s = 0.f;
        if (active)
            for (int c = 0; c < C; ++c) s = fmaf(a(c, true), prob(h, c, lse), s);
        store(h, dst, C, active, [&](int c) { return g(prob(h, c, lse), a(c, true), s); });
    }
};

// The pixel's CE gradient g[c] = w * (softmax[c] - onehot[c]).
template <typename T, int CS8>
__device__ __forceinline__ void ce_grad_store(T* __restrict__ dst, const typename Pixel<T, CS8>::Held& h, float lse, float w, int lab, int C,
                                              bool active) {
    Pixel<T, CS8>::store(h, dst, C, active, [&](int c) { return w * (Pixel<T, CS8>::prob(h, c, lse) - (c == lab ? 1.f : 0.f)); });
}

// The focal loss as two factors on the CE weight w of an active pixel (msau_focal_factor, loss_cost.h): the loss term is
// wl * nll, the gradient wg * (softmax - onehot).  xl: the pixel's logit at its label.  gamma = 0 leaves w in both, bit for bit.
__device__ __forceinline__ void focal_weights(float w, float lse, float xl, float gamma, float& wl, float& wg) {
    float f, m;
    msau_focal_factor(__expf(xl - lse), lse - xl, gamma, &f, &m);
    wl = w * f;
    wg = w * m;
}

// The workgroup sum, reproducible, in two halves so that several values share one barrier: wave_sum adds the lanes of a wave by
// shuffle-down and leaves the wave's total in red[wave]; after a barrier add_waves adds the NW totals -- in index order from zero,
// or PAIRED as (r0 + r1) + (r2 + r3).  Which of the two a kernel uses is part of its result's bits.
template <typename V>
__device__ __forceinline__ void wave_sum(V v, V* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
}
template <int NW, bool PAIRED, typename V>
__device__ __forceinline__ V add_waves(const V* red) {
    if constexpr (PAIRED) {
        static_assert(NW == 4, "the paired order is that of four waves");
        return (red[0] + red[1]) + (red[2] + red[3]);
    } else {
        V s = 0;
        for (int i = 0; i < NW; ++i) s += red[i];
        return s;
    }
}
// one value: the total comes back to thread 0 (zero to every other thread)
template <int NW, bool PAIRED, typename V>
__device__ __forceinline__ V block_sum(V v, V* red) {
    wave_sum(v, red);
    __syncthreads();
    return threadIdx.x == 0 ? add_waves<NW, PAIRED>(red) : V(0);
}

constexpr int kWaves = kThreads / 64;                                // of the 256-thread CE kernels

// =============================================================================================
// masked cross entropy (model/model.py:446-459), batch rule of SURVEY 8(e)
// =============================================================================================
// One 1024-thread workgroup per sample, 16-byte loads (two labels), eight in flight per thread, no atomics and no
// memset: counts[b] is written, not accumulated.  (The first version spread a sample over 64 workgroups and let every
// wave atomicAdd into counts[b]: 4096 same-address atomics took 51 us for 11 MB of labels.)
__global__ __launch_bounds__(1024) void label_count_kernel(const int64_t* __restrict__ labels, int32_t* __restrict__ counts, int64_t hw) {
    __shared__ int red[16];
    const int b = blockIdx.x;
    const int64_t* base = labels + (int64_t)b * hw;
    int local = 0;
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    const int64_t npair = hw >> 1;                                   // base is 16-byte aligned when hw is even or b == 0
    const bool aligned = ((reinterpret_cast<uintptr_t>(base) & 15) == 0);
    if (aligned) {
        const ll2* p2 = reinterpret_cast<const ll2*>(base);
        int64_t i = threadIdx.x;
        for (; i + 7 * 1024 < npair; i += 8 * 1024) {
            ll2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p2[i + u * 1024];
#pragma unroll
            for (int u = 0; u < 8; ++u) local += (v[u][0] > 0) + (v[u][1] > 0);
        }
        for (; i < npair; i += 1024) { ll2 v = p2[i]; local += (v[0] > 0) + (v[1] > 0); }
        if ((hw & 1) && threadIdx.x == 0) local += base[hw - 1] > 0;
    } else {
        for (int64_t i = threadIdx.x; i < hw; i += 1024) local += base[i] > 0;
    }
    const int t = block_sum<16, false>(local, red);
    if (threadIdx.x == 0) counts[b] = t;
}

// The same count with a sample spread over K workgroups (grid K x B): partial[b * K + k] is written, the consumer
// (msau_masked_ce_multi with counts_k = K) adds the K integers up -- exact in any order, no atomics, no follow-up launch.  One
// workgroup per sample left 240 of 256 CUs idle: 15 us for the bench's 11 MB of labels, on the main queue between the sweeps.
__global__ __launch_bounds__(256) void label_count_split_kernel(const int64_t* __restrict__ labels, int32_t* __restrict__ partial,
                                                                int64_t hw, int K) {
    __shared__ int red[4];
    const int b = blockIdx.y, k = blockIdx.x;
    const int64_t chunk = (hw + K - 1) / K;
    const int64_t lo = (int64_t)k * chunk, hi = lo + chunk < hw ? lo + chunk : hw;
    const int64_t* base = labels + (int64_t)b * hw;
    int local = 0;
    int64_t i = lo + threadIdx.x;
    for (; i + 7 * 256 < hi; i += 8 * 256) {
        int64_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = base[i + u * 256];
#pragma unroll
        for (int u = 0; u < 8; ++u) local += v[u] > 0;
    }
    for (; i < hi; i += 256) local += base[i] > 0;
    const int t = block_sum<4, true>(local, red);
    if (threadIdx.x == 0) partial[b * K + k] = t;
}

// the block's loss partial -> partials[blockIdx.x]; with class weights (the weighted CE) the block's sum of weights, reduced in
// the same order, -> partials[gridDim.x + blockIdx.x]
__device__ __forceinline__ void ce_block_sums(float local, float local_w, bool weighted, float* red, float* __restrict__ partials) {
    const float s = block_sum<kWaves, false>(local, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
    if (weighted) {
        __syncthreads();
        const float sw = block_sum<kWaves, false>(local_w, red);
        if (threadIdx.x == 0) partials[gridDim.x + blockIdx.x] = sw;
    }
}

// One head; the host takes the register form up to 16 stored channels and the cache form beyond (e.g. the 17-class key-value head).
// ALL: every label in [0, C) counts and the weight is `scale` (plain softmax CE); otherwise the labels in [1, C) count with
// scale / counts[b].
// cw (ALL only): per-class weights of torch.nn.CrossEntropyLoss(weight) (model/training/cost.py:24-31): every pixel's term and
// gradient are multiplied by cw[label]; the sum of those weights -- the loss's denominator -- goes to the second half of partials
template <typename T, bool ALL, int CS8>
__global__ void masked_ce_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                                 const int32_t* __restrict__ counts, T* __restrict__ dlogits, float* __restrict__ partials,
                                 int B, int64_t hw, int C, float scale, const float* __restrict__ cw, int Cs) {
    using Px = Pixel<T, CS8>;
    const int cs = Px::kCs ? Px::kCs : Cs;                             // a pixel's stride: stated as a constant in the register form
    __shared__ float red[kWaves];
    float local = 0.f, local_w = 0.f;
    const int64_t total = (int64_t)B * hw;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(p / hw);
        const int64_t lab = labels[p];
        const bool on = ALL ? (lab >= 0 && lab < C) : (lab > 0 && lab < C);
        float w = on ? (ALL ? scale : scale / (float)max(counts[b], 1)) : 0.f;
        if (ALL && cw && on) { const float c = cw[(int)lab]; w *= c; local_w += c; }
        typename Px::Held h;
        float xl;
        const float lse = Px::load(h, logits + p * cs, Cs, C, (int)lab, xl);
        xl = Px::label_logit(h, (int)lab, on, xl);
        if (on) local += w * (lse - xl);
        ce_grad_store<T, CS8>(dlogits + p * cs, h, lse, w, (int)lab, C, on);
    }
    ce_block_sums(local, local_w, ALL && cw, red, partials);
}

constexpr int kCeMaxB = 1024;
// Final + auxiliary masked CE in ONE launch (model/model.py:455-458: CE(out) + CE(aux) over the same labelled pixels):
// the label and the per-sample weight are read once, both gradients are written, block partial sums go to ws and the
// one-wave follow-up kernel adds them up in index order -> loss[0], reproducibly.  (A "last block sums" ticket
// instead of the second launch was tried: thousands of same-address atomics cost 200 us.)
template <typename T, int NL, int CS8>
__global__ void masked_ce_multi_kernel(const T* __restrict__ l0, const T* __restrict__ l1, const int64_t* __restrict__ labels,
                                       const int32_t* __restrict__ counts, T* __restrict__ d0, T* __restrict__ d1,
                                       float* __restrict__ ws, float* __restrict__ loss, int B, int hw, int C, float scale, int K) {
    using Px = Pixel<T, CS8>;
    constexpr int Cs = CS8 * 8;
    __shared__ float red[kWaves];
    __shared__ int cnt[kCeMaxB];                                       // per-sample counts: the K partial counts added up (B <= kCeMaxB)
    const bool in_lds = B <= kCeMaxB;
    if (in_lds) {
        for (int b = threadIdx.x; b < B; b += blockDim.x) {
            int t = 0;
            for (int k = 0; k < K; ++k) t += counts[b * K + k];
            cnt[b] = t;
        }
        __syncthreads();
    }
    float local = 0.f;
    const int64_t total = (int64_t)B * hw;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)((unsigned)p / (unsigned)hw);               // total < 2^31 (checked by the host)
        const int lab = (int)labels[p];
        const bool on = lab != 0 && lab < C && lab > 0;
        const float w = on ? scale / (float)max(in_lds ? cnt[b] : counts[b], 1) : 0.f;
#pragma unroll
        for (int t = 0; t < NL; ++t) {
            typename Px::Held h;
            float xl;
            const float lse = Px::load(h, (t ? l1 : l0) + p * Cs, Cs, C, lab, xl);
            if (on) local += w * (lse - xl);
            ce_grad_store<T, CS8>((t ? d1 : d0) + p * Cs, h, lse, w, lab, C, on);
        }
    }
    const float s = block_sum<kWaves, false>(local, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// 256 threads, fixed association order (thread t adds elements t, t+256, ...; lanes, then waves, combine in index
// order) -> reproducible.  SET overwrites out[0], otherwise out[0] += sum.
template <bool SET>
__global__ __launch_bounds__(256) void ordered_sum_kernel_t(const float* __restrict__ partials, int n, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
    const float t = block_sum<4, true>(s, red);
    if (threadIdx.x == 0) {
        if (SET) out[0] = t; else out[0] += t;
    }
}

// =============================================================================================
// UNetLoss for a (ragged) batch of documents (model/training/cost.py:35-65): plain CE over every pixel of a document, class 0
// counted, 0.5 * final + 0.5 * auxiliary, optional class weights; every head has its own label map
// =============================================================================================
constexpr int kHistMaxC = 256;
// Class histogram of the labelled pixels of a document: grid K x B, a document's pixels shared out over its K workgroups, one LDS
// histogram per wavefront (LDS atomics only), partial[(b * K + k) * C + c] is WRITTEN.  The consumer adds the K rows: exact in any order.
__global__ __launch_bounds__(256) void label_hist_kernel(const int64_t* __restrict__ labels, const int32_t* __restrict__ extent,
                                                         int32_t* __restrict__ partial, int H, int W, int C, int K) {
    __shared__ int hist[4][kHistMaxC];
    const int b = blockIdx.y, k = blockIdx.x, wv = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 4 * kHistMaxC; i += 256) (&hist[0][0])[i] = 0;
    __syncthreads();
    const int hw = H * W;                                            // B * H * W < 2^31 (checked by the host)
    const int eh = extent ? min(max(extent[2 * b], 0), H) : H, ew = extent ? min(max(extent[2 * b + 1], 0), W) : W;
    const int chunk = (hw + K - 1) / K;
    const int lo = k * chunk, hi = min(lo + chunk, hw);
    const int64_t* base = labels + (int64_t)b * hw;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const int64_t lab = base[i];
        if (lab >= 0 && lab < C && pos_in_extent(i, W, eh, ew)) atomicAdd(&hist[wv][(int)lab], 1);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256)
        partial[((int64_t)b * K + k) * C + c] = (hist[0][c] + hist[1][c]) + (hist[2][c] + hist[3][c]);
}

// inv[t * B + b] = 1 / (B * D_b(head t)), 0 for a document without weight: D_b is the extent's area, or with class weights
// sum_c cw[c] * hist_t[b][c], the classes added in index order (hist_t = hist + t * B * K * C, its K rows added first)
// MASKED (the masked cost: one label map, the classes from 1): always from the one histogram, D_b = sum_{c >= 1} cw[c] * hist[b][c]
// (cw absent: the number of labelled pixels); the caller passes NL = 1
template <bool MASKED>
__device__ __forceinline__ void unet_ce_denominators(float* inv, const int32_t* __restrict__ extent, const float* __restrict__ cw,
                                                     const int32_t* __restrict__ hist, int NL, int B, int H, int W, int C, int K) {
    for (int i = threadIdx.x; i < NL * B; i += blockDim.x) {
        const int t = i / B, b = i - t * B;
        float d;
        if (MASKED || cw) {
            const int32_t* h = hist + ((int64_t)t * B + b) * K * C;
            d = 0.f;
            for (int c = MASKED ? 1 : 0; c < C; ++c) {
                int n = 0;
                for (int k = 0; k < K; ++k) n += h[k * C + c];
                d += (cw ? cw[c] : 1.f) * (float)n;
            }
        } else {
            const int eh = extent ? min(max(extent[2 * b], 0), H) : H, ew = extent ? min(max(extent[2 * b + 1], 0), W) : W;
            d = (float)eh * (float)ew;
        }
        inv[i] = d > 0.f ? 1.f / ((float)B * d) : 0.f;
    }
    __syncthreads();
}

// the block's two sums -> ws[blockIdx.x] (final), ws[gridDim.x + blockIdx.x] (auxiliary); one barrier for both
__device__ __forceinline__ void unet_ce_block_sums(float l0, float l1, float* red, float* __restrict__ ws) {
    wave_sum(l0, red);
    wave_sum(l1, red + kWaves);
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[blockIdx.x] = add_waves<kWaves, false>(red);
        ws[gridDim.x + blockIdx.x] = add_waves<kWaves, false>(red + kWaves);
    }
}

// Both heads in one launch; the host takes the register form up to 32 stored channels and the cache form beyond.
// A thread's weight of head t at pixel p of document b: hw_t * cw[lab] / (B * D_b(t)) inside the extent with lab in [0, C), else 0;
// the loss partials carry the weight WITHOUT hw_t (loss3[1], loss3[2] are the heads' own losses).
// FOCAL: the focal loss with parameter gamma (focal_weights); otherwise gamma is not read.
// MASKED: the masked cost of TrainEngine.step -- both heads against lab0, whose label, extent test and weight are
// taken once per pixel; the active classes start at 1; the head weight is 1.
template <typename T, int NL, int CS8, bool FOCAL, bool MASKED>
__global__ void unet_ce_kernel(const T* __restrict__ l0, const T* __restrict__ l1, const int64_t* __restrict__ lab0,
                               const int64_t* __restrict__ lab1, const int32_t* __restrict__ extent, const float* __restrict__ cw,
                               const int32_t* __restrict__ hist, int K, T* __restrict__ d0, T* __restrict__ d1,
                               float* __restrict__ ws, int B, int H, int W, int C, float gamma, int Cs) {
    using Px = Pixel<T, CS8>;
    const int cs = Px::kCs ? Px::kCs : Cs;                             // a pixel's stride: stated as a constant in the register form
    __shared__ float red[2 * kWaves];
    __shared__ float inv[2 * kCeMaxB];
    constexpr int kHeadUnroll = NL ? NL : 1;                           // NL = 0 (the cache form): the head count is read at run time, the loop stays a loop
    const int nl = NL ? NL : (l1 ? 2 : 1);
    unet_ce_denominators<MASKED>(inv, extent, cw, hist, MASKED ? 1 : nl, B, H, W, C, K);
    const float hwt = (nl == 2 && !MASKED) ? 0.5f : 1.f;
    const int hw = H * W;
    float local[2] = {0.f, 0.f};
    const int64_t total = (int64_t)B * hw;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)((unsigned)p / (unsigned)hw);               // total < 2^31 (checked by the host)
        const int j = (int)p - b * hw;
        const bool in = extent ? pos_in_extent(j, W, extent[2 * b], extent[2 * b + 1]) : true;
        bool on = false;
        int lab = -1;
        float w = 0.f;
#pragma unroll kHeadUnroll
        for (int t = 0; t < nl; ++t) {
            if (!MASKED || t == 0) {
                const int64_t lab64 = (t ? lab1 : lab0)[p];
                on = in && lab64 >= (MASKED ? 1 : 0) && lab64 < C;
                lab = on ? (int)lab64 : -1;
                w = on ? inv[t * B + b] * (cw ? cw[lab] : 1.f) : 0.f;
            }
            typename Px::Held h;
            float xl;
            const float lse = Px::load(h, (t ? l1 : l0) + p * cs, Cs, C, lab, xl);
            const bool act = on && w != 0.f;
            xl = Px::label_logit(h, lab, act, xl);
            float wl = w, wg = w;
            if (FOCAL && act) focal_weights(w, lse, xl, gamma, wl, wg);
            if (act) local[t] += wl * (lse - xl);
            ce_grad_store<T, CS8>((t ? d1 : d0) + p * cs, h, lse, hwt * wg, lab, C, act);
        }
    }
    unet_ce_block_sums(local[0], local[1], red, ws);
}

// the follow-up: the block partials of each head added in ordered_sum_kernel_t's order -> loss3 = (total, final, auxiliary), written
// MASKED: the total is final + auxiliary (head weights 1 and 1)
template <bool MASKED>
__global__ __launch_bounds__(256) void unet_ce_finish_kernel(const float* __restrict__ ws, int n, int two, float* __restrict__ loss3) {
    __shared__ float red[8];
    float s0 = 0.f, s1 = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { s0 += ws[i]; s1 += ws[n + i]; }
    wave_sum(s0, red);
    wave_sum(s1, red + 4);
    __syncthreads();
    if (threadIdx.x == 0) {
        const float f = add_waves<4, true>(red);
        const float a = two ? add_waves<4, true>(red + 4) : 0.f;
        if (MASKED) loss3[0] = two ? f + a : f;
        else loss3[0] = two ? 0.5f * f + 0.5f * a : f;
        loss3[1] = f;
        loss3[2] = a;
    }
}

// =============================================================================================
// UNetLoss and the reference's accuracy, forward only and per document (validation: model/training/trainer.py's epoch print,
// cost.py:44-48 `non_zero_mask`).  Grid K x B as label_hist_kernel: workgroup k of document b takes rows [k * rpk, (k + 1) * rpk) of
// the document's extent, rpk = ceil(h_b / K), and WRITES one partial row; nothing outside the extent is read.
// =============================================================================================
struct UnetEvalRow { float num[2], den[2]; int32_t cnt[2][2]; };    // per head: sum cw * nll, sum cw; (labelled, correct)

// one pixel of one head into the thread's sums.  lse / xl: the pixel's log-sum-exp and its logit at the label; pred: its first maximum
// FOCAL: the numerator takes the focal term (focal_weights), the denominator stays CE's
template <bool FOCAL>
__device__ __forceinline__ void unet_eval_add(int lab, bool on, float lse, float xl, int pred, const float* __restrict__ cw, float gamma,
                                              float& num, float& den, int& labelled, int& correct) {
    if (!on) return;
    const float w = cw ? cw[lab] : 1.f;
    den += w;
    float wl = w, wg = w;
    if (FOCAL && w != 0.f) focal_weights(w, lse, xl, gamma, wl, wg);
    if (w != 0.f) num += wl * (lse - xl);
    if (lab >= 1) { labelled += 1; correct += pred == lab; }
}

// the workgroup's eight sums -> its row: lanes, then the four waves paired (reproducible).  Not wave_sum / add_waves: a wave's eight
// totals go to LDS as two 16-byte rows and thread i < 4 adds up value i; with the shared form (eight strided columns) the
// evaluation kernels measured 1.5 - 3 % slower (profiles/loss_refactor.md)
__device__ __forceinline__ void unet_eval_block_row(float (&num)[2], float (&den)[2], int (&cnt)[2][2], UnetEvalRow* __restrict__ row) {
    __shared__ float redf[4][4];
    __shared__ int redi[4][4];
    float f[4] = {num[0], num[1], den[0], den[1]};
    int n[4] = {cnt[0][0], cnt[0][1], cnt[1][0], cnt[1][1]};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        for (int o = 32; o > 0; o >>= 1) { f[i] += __shfl_down(f[i], o, 64); n[i] += __shfl_down(n[i], o, 64); }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { redf[threadIdx.x >> 6][i] = f[i]; redi[threadIdx.x >> 6][i] = n[i]; }
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int i = threadIdx.x;
        const float fs = (redf[0][i] + redf[1][i]) + (redf[2][i] + redf[3][i]);
        const int ns = (redi[0][i] + redi[1][i]) + (redi[2][i] + redi[3][i]);
        (i < 2 ? row->num : row->den)[i & 1] = fs;
        row->cnt[i >> 1][i & 1] = ns;
    }
}

// the slab of workgroup k: pixel i of it -> canvas offset of the pixel inside document b, false past the slab's end
struct UnetEvalSlab {
    int r0, n, ew;
    __device__ __forceinline__ UnetEvalSlab(const int32_t* __restrict__ extent, int b, int k, int K, int H, int W) {
        const int eh = extent ? min(max(extent[2 * b], 0), H) : H;
        ew = extent ? min(max(extent[2 * b + 1], 0), W) : W;
        const int rpk = (eh + K - 1) / K;
        r0 = min(k * rpk, eh);
        n = (min(r0 + rpk, eh) - r0) * ew;                            // <= H * W < 2^31 (checked by the host)
    }
    __device__ __forceinline__ int offset(int i, int W) const { const int y = i / ew; return (r0 + y) * W + (i - y * ew); }
};

// MASKED: both heads against lab0, read once; the active classes start at 1
template <typename T, int NL, int CS8, bool FOCAL, bool MASKED>
__global__ __launch_bounds__(256) void unet_eval_kernel(const T* __restrict__ l0, const T* __restrict__ l1,
                                                        const int64_t* __restrict__ lab0, const int64_t* __restrict__ lab1,
                                                        const int32_t* __restrict__ extent, const float* __restrict__ cw,
                                                        UnetEvalRow* __restrict__ rows, int H, int W, int C, float gamma, int Cs) {
    using Px = Pixel<T, CS8>;
    const int cs = Px::kCs ? Px::kCs : Cs;                             // a pixel's stride: stated as a constant in the register form
    constexpr int kChannelUnroll = Px::kUnroll;
    constexpr int kHeadUnroll = NL ? NL : 1;                           // NL = 0 (the cache form): the head count is read at run time, the loop stays a loop
    const int nl = NL ? NL : (l1 ? 2 : 1);
    const int b = blockIdx.y, k = blockIdx.x, K = gridDim.x;
    const UnetEvalSlab slab(extent, b, k, K, H, W);
    const int64_t base = (int64_t)b * H * W;
    float num[2] = {0.f, 0.f}, den[2] = {0.f, 0.f};
    int cnt[2][2] = {{0, 0}, {0, 0}};
    for (int i = threadIdx.x; i < slab.n; i += 256) {
        const int64_t p = base + slab.offset(i, W);
        bool on = false;
        int lab = -1;
#pragma unroll kHeadUnroll
        for (int t = 0; t < nl; ++t) {
            if (!MASKED || t == 0) {
                const int64_t lab64 = (t ? lab1 : lab0)[p];
                on = lab64 >= (MASKED ? 1 : 0) && lab64 < C;
                lab = on ? (int)lab64 : -1;
            }
            typename Px::Held h;
            float xl;
            const float lse = Px::load(h, (t ? l1 : l0) + p * cs, Cs, C, lab, xl);
            xl = Px::label_logit(h, lab, on, xl);
            int pred = 0;
            float bv = -INFINITY;
#pragma unroll kChannelUnroll
            for (int c = 0; c < Px::channels(C); ++c)
                if (c < C) first_max(Px::logit(h, c), c, bv, pred);
            unet_eval_add<FOCAL>(lab, on, lse, xl, pred, cw, gamma, num[t], den[t], cnt[t][0], cnt[t][1]);
        }
    }
    unet_eval_block_row(num, den, cnt, rows + (int64_t)b * K + k);
}

// the follow-up: one thread per (document, head) adds the document's K rows in index order and divides; every output is written
__global__ __launch_bounds__(256) void unet_eval_finish_kernel(const UnetEvalRow* __restrict__ rows, int B, int K,
                                                               float* __restrict__ doc_loss, int32_t* __restrict__ doc_counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * B) return;
    const int b = i >> 1, t = i & 1;
    float n = 0.f, d = 0.f;
    int labelled = 0, correct = 0;
    for (int k = 0; k < K; ++k) {
        const UnetEvalRow& r = rows[(int64_t)b * K + k];
        n += r.num[t];
        d += r.den[t];
        labelled += r.cnt[t][0];
        correct += r.cnt[t][1];
    }
    doc_loss[i] = d > 0.f ? n / d : 0.f;
    doc_counts[2 * i] = labelled;
    doc_counts[2 * i + 1] = correct;
}

// =============================================================================================
// the soft Dice loss under UNetLoss's rules: per document and class the sums I_c = sum p_c [y = c] and P_c = sum p_c
// over the active pixels (unet_dice_sums_kernel, grid K x B over the slabs of unet_eval_kernel), the coefficient step
// (unet_dice_coef_kernel: the K rows in index order, Y_c from msau_label_hist's rows, msau_dice_coef of loss_cost.h), and for
// training the gradient pass (unet_dice_grad_kernel, of unet_ce_kernel's shape) that reads the (hit, miss) table from global memory.
// =============================================================================================
// The workgroup's sums of N classes -> row[0][c0 + c] = I, row[1][c0 + c] = P (row: [2][C]) for c0 + c < C: lanes by shuffle, the four
// waves paired.  red: 2 * N * 4 floats; may be called again after it returns.
template <int N>
__device__ __forceinline__ void dice_block_rows(const float (&I)[N], const float (&P)[N], float* red, float* __restrict__ row, int c0, int C) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
        wave_sum(I[c], red + (2 * c) * 4);
        wave_sum(P[c], red + (2 * c + 1) * 4);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * N; i += 256) {
        const int c = c0 + (i >> 1);
        if (c < C) row[(i & 1) * C + c] = add_waves<4, true>(red + i * 4);
    }
    __syncthreads();
}

// part[((t * B + b) * K + k)][2][C] is WRITTEN by workgroup k of document b for head t; a thread adds its pixels in slab order,
// Pixel::kDiceChunk classes per sweep of the slab (the register form: all of them in one sweep)
// MASKED: both heads against lab0; the active classes start at 1 (I_0 = 0, P_0 is summed as every class's)
template <typename T, int NL, int CS8, bool MASKED>
__global__ __launch_bounds__(256) void unet_dice_sums_kernel(const T* __restrict__ l0, const T* __restrict__ l1,
                                                             const int64_t* __restrict__ lab0, const int64_t* __restrict__ lab1,
                                                             const int32_t* __restrict__ extent, float* __restrict__ part, int B, int H,
                                                             int W, int C, int Cs) {
    using Px = Pixel<T, CS8>;
    const int cs = Px::kCs ? Px::kCs : Cs;                             // a pixel's stride: stated as a constant in the register form
    constexpr int N = Px::kDiceChunk;
    __shared__ float red[2 * N * 4];
    constexpr int kHeadUnroll = NL ? NL : 1;                           // NL = 0 (the cache form): the head count is read at run time, the loop stays a loop
    const int nl = NL ? NL : (l1 ? 2 : 1);
    const int b = blockIdx.y, k = blockIdx.x, K = gridDim.x;
    const UnetEvalSlab slab(extent, b, k, K, H, W);
    const int64_t base = (int64_t)b * H * W;
#pragma unroll kHeadUnroll
    for (int t = 0; t < nl; ++t) {
        for (int sweep = 0; sweep < Px::dice_sweeps(C); ++sweep) {
            const int c0 = sweep * N;
            float I[N], P[N];
#pragma unroll
            for (int c = 0; c < N; ++c) I[c] = P[c] = 0.f;
            for (int i = threadIdx.x; i < slab.n; i += 256) {
                const int64_t p = base + slab.offset(i, W);
                const int64_t lab64 = (t && !MASKED ? lab1 : lab0)[p];
                if (lab64 < (MASKED ? 1 : 0) || lab64 >= C) continue;
                const int lab = (int)lab64;
                typename Px::Held h;
                float xl;
                const float lse = Px::load(h, (t ? l1 : l0) + p * cs, Cs, C, lab, xl);
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    const float pc = c0 + c < C ? Px::prob(h, c0 + c, lse) : 0.f;
                    P[c] += pc;
                    I[c] += c0 + c == lab ? pc : 0.f;
                }
            }
            dice_block_rows<N>(I, P, red, part + (((int64_t)t * B + b) * K + k) * 2 * C, c0, C);
        }
    }
}

// The coefficient step: grid (B, heads), thread c takes class c (C <= 256).  The K rows of `part` and the Kh rows of the head's label
// histogram are added in index order; tab[(t * B + b) * C + c] = (hit, miss) when tab is given; the document's loss, the classes
// added lanes-then-waves, times `scale` -> doc_loss[b * sb + t * st].  Every output is written.
// MASKED: one histogram for both heads, Y_0 = 0 whatever the histogram counted at label 0, and a document without a labelled pixel
// has loss 0 (its table is unread: no pixel of it is active).
template <bool MASKED>
__global__ __launch_bounds__(256) void unet_dice_coef_kernel(const float* __restrict__ part, int K, const int32_t* __restrict__ hist, int Kh,
                                                             const float* __restrict__ cw, float eps, float2* __restrict__ tab,
                                                             float* __restrict__ doc_loss, int sb, int st, float scale, int B, int C) {
    __shared__ float red[4];
    const int b = blockIdx.x, t = blockIdx.y, c = threadIdx.x;
    float V = 0.f;                                                   // every thread the same sum, classes in index order
    for (int i = 0; i < C; ++i) V += cw ? cw[i] : 1.f;
    float term = 0.f;
    int n = 0;
    if (c < C) {
        const float* rows = part + ((int64_t)t * B + b) * K * 2 * C;
        const int32_t* h = hist + ((int64_t)(MASKED ? 0 : t) * B + b) * Kh * C;
        float I = 0.f, P = 0.f;
        for (int k = 0; k < K; ++k) { I += rows[(int64_t)k * 2 * C + c]; P += rows[(int64_t)k * 2 * C + C + c]; }
        for (int k = 0; k < Kh; ++k) n += h[k * C + c];
        if (MASKED && c == 0) n = 0;
        float hit, miss;
        msau_dice_coef(I, P, (float)n, eps, V > 0.f ? (cw ? cw[c] : 1.f) / V : 0.f, &term, &hit, &miss);
        if (tab) tab[((int64_t)t * B + b) * C + c] = make_float2(hit, miss);
    }
    const bool labelled = MASKED ? __syncthreads_or(n > 0) != 0 : true;
    const float s = block_sum<4, true>(term, red);
    if (threadIdx.x == 0) doc_loss[b * sb + t * st] = labelled ? scale * msau_dice_loss(V, s) : 0.f;
}

// The pixel's Dice gradient g[j] = sc * p_j * (a_j - sum_c a_c p_c), a_c = hit_c at the label, else miss_c (tab: the document's C
// (hit, miss) pairs).
template <typename T, int CS8>
__device__ __forceinline__ void dice_grad_store(T* __restrict__ dst, typename Pixel<T, CS8>::Held& h, float lse, const float2* __restrict__ tab, float sc, int lab,
                                                int C, bool active) {
    // (the table entry is selected from outside the condition it is loaded under: the loads of a pixel's channels stay in flight together)
    Pixel<T, CS8>::store_dot(h, dst, lse, C, active, [&](int c, bool real) { const float2 hm = real ? tab[c] : make_float2(0.f, 0.f); return c == lab ? hm.x : hm.y; },
                 [&](float p, float a, float s) { return sc * (p * (a - s)); });
}

// The gradient pass, of unet_ce_kernel's shape: every pixel of the canvas, both heads, sc = head weight / B
// MASKED: as in unet_ce_kernel -- lab0 read once for both heads, the active classes from 1, head weight 1
template <typename T, int NL, int CS8, bool MASKED>
__global__ void unet_dice_grad_kernel(const T* __restrict__ l0, const T* __restrict__ l1, const int64_t* __restrict__ lab0,
                                      const int64_t* __restrict__ lab1, const int32_t* __restrict__ extent, const float2* __restrict__ tab,
                                      T* __restrict__ d0, T* __restrict__ d1, int B, int H, int W, int C, int Cs) {
    using Px = Pixel<T, CS8>;
    const int cs = Px::kCs ? Px::kCs : Cs;                             // a pixel's stride: stated as a constant in the register form
    constexpr int kHeadUnroll = NL ? NL : 1;                           // NL = 0 (the cache form): the head count is read at run time, the loop stays a loop
    const int nl = NL ? NL : (l1 ? 2 : 1);
    const float sc = ((nl == 2 && !MASKED) ? 0.5f : 1.f) / (float)B;
    const int hw = H * W;
    const int64_t total = (int64_t)B * hw;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)((unsigned)p / (unsigned)hw);               // total < 2^31 (checked by the host)
        const int j = (int)p - b * hw;
        const bool in = extent ? pos_in_extent(j, W, extent[2 * b], extent[2 * b + 1]) : true;
        bool on = false;
        int lab = -1;
#pragma unroll kHeadUnroll
        for (int t = 0; t < nl; ++t) {
            if (!MASKED || t == 0) {
                const int64_t lab64 = (t ? lab1 : lab0)[p];
                on = in && lab64 >= (MASKED ? 1 : 0) && lab64 < C;
                lab = on ? (int)lab64 : -1;
            }
            typename Px::Held h;
            float xl;
            const float lse = Px::load(h, (t ? l1 : l0) + p * cs, Cs, C, lab, xl);
            dice_grad_store<T, CS8>((t ? d1 : d0) + p * cs, h, lse, tab + ((int64_t)t * B + b) * C, sc, lab, C, on);
        }
    }
}

// Evaluation counts (the per-epoch accuracy / classification report of train_chargrid_funsd_msau.py): for every pixel whose
// label is in [1, C) (and, with `extent`, that lies inside its sample's extent) pred = the first maximum of the C stored logits
// (torch's argmax of the fp32 export, ties included), 0 -> zero_as when zero_as >= 0, and counts[label * C + pred] += 1.
// A workgroup histograms into LDS (uint32 bins) and adds each non-empty bin to the int64 matrix with one global atomic:
// integer sums, so the result does not depend on arrival order.
constexpr int kConfusionMaxC = 64;

template <typename T>
__global__ __launch_bounds__(256) void eval_confusion_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                             unsigned long long* __restrict__ counts, int64_t npix, int H, int W,
                                                             int C, int Cs, int zero_as, const int32_t* __restrict__ extent) {
    __shared__ uint32_t hist[kConfusionMaxC * kConfusionMaxC];
    const int bins = C * C;
    for (int i = threadIdx.x; i < bins; i += blockDim.x) hist[i] = 0u;
    __syncthreads();
    const int64_t hw = (int64_t)H * W;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lab = labels[p];
        if (lab < 1 || lab >= C) continue;
        if (extent) {
            const int b = (int)(p / hw);
            const int64_t r = p - (int64_t)b * hw;
            const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
            if (y >= extent[2 * b] || x >= extent[2 * b + 1]) continue;
        }
        const T* l = logits + p * Cs;
        int best = 0;
        float bv = -INFINITY;
        for (int c0 = 0; c0 < C; c0 += 8) {
            const typename Vec8<T>::type v8 = load8<T>(l + c0);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (c0 + j < C) first_max((float)v8[j], c0 + j, bv, best);
            }
        }
        if (best == 0 && zero_as >= 0) best = zero_as;
        atomicAdd(&hist[(int)lab * C + best], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += blockDim.x) {
        const uint32_t n = hist[i];
        if (n) atomicAdd(counts + i, (unsigned long long)n);
    }
}

// =============================================================================================
// the softmax heads.  Three statements of one head -- these two and msau_head_softmax() of msau_common.h, which the conv epilogues
// of other translation units inline -- with the same operations in the same order (max, sum and product in channel order, __expf);
// tests/test_inference_gpu.py pins their agreement.
// =============================================================================================
__global__ void softmax_nchw_kernel(const float* __restrict__ logits, float* __restrict__ pred, int B, int C, int64_t hw) {
    const int64_t total = (int64_t)B * hw;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t b = i / hw, p = i % hw;
        const float* src = logits + b * C * hw + p;
        float mx = -INFINITY;
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, src[c * hw]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += __expf(src[c * hw] - mx);
        float inv = 1.f / se;
        for (int c = 0; c < C; ++c) pred[b * C * hw + c * hw + p] = __expf(src[c * hw] - mx) * inv;
    }
}

// softmax + first-maximum index over the C real channels of NHWC logits, any C <= 255.  Operation for operation
// msau_head_softmax() of msau_common.h, which the conv epilogue (MSAU_CONV_HEAD) uses for C <= 16: the two produce identical bits.
template <typename T>
__global__ void softmax_argmax_nhwc_kernel(const T* __restrict__ logits, float* __restrict__ probs,
                                           uint8_t* __restrict__ amax, int64_t npix, int C, int Cs) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        const T* l = logits + p * Cs;
        float mx = -INFINITY;
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, (float)l[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += __expf((float)l[c] - mx);
        const float inv = 1.f / se;
        int best = 0;
        float bp = -1.f;
        for (int c = 0; c < C; ++c) {
            const float pr = __expf((float)l[c] - mx) * inv;
            probs[p * C + c] = pr;
            if (pr > bp) { bp = pr; best = c; }
        }
        amax[p] = (uint8_t)best;
    }
}

}  // namespace

// The family's instance ladder, stated once: dtype -> T, a second head -> NL = 2, Cs -> the register form with Cs = 8 * CS8, or
// what lies beyond it (the cache form, CS8 = 0, where there is one: it reads the head count at run time, NL = 0).  LAUNCH(T, NL, CS8)
// is the caller's one launch expression.
#define LOSS_FORM(dtype, two, LAUNCH, C8)                                                 \
    do {                                                                                  \
        if (two) { DISPATCH_T(dtype, LAUNCH(float, 2, C8), LAUNCH(bf16_t, 2, C8)); }      \
        else { DISPATCH_T(dtype, LAUNCH(float, 1, C8), LAUNCH(bf16_t, 1, C8)); }          \
    } while (0)
#define LOSS_CACHE(dtype, LAUNCH) DISPATCH_T(dtype, LAUNCH(float, 0, 0), LAUNCH(bf16_t, 0, 0))
#define LOSS_LADDER_16(dtype, two, Cs, LAUNCH, BEYOND)                                    \
    do {                                                                                  \
        if ((Cs) == 8) LOSS_FORM(dtype, two, LAUNCH, 1);                                  \
        else if ((Cs) == 16) LOSS_FORM(dtype, two, LAUNCH, 2);                            \
        else { BEYOND; }                                                                  \
    } while (0)
#define LOSS_LADDER_32(dtype, two, Cs, LAUNCH)                                            \
    LOSS_LADDER_16(dtype, two, Cs, LAUNCH,                                                \
                   if ((Cs) == 24) LOSS_FORM(dtype, two, LAUNCH, 3);                      \
                   else if ((Cs) == 32) LOSS_FORM(dtype, two, LAUNCH, 4);                 \
                   else LOSS_CACHE(dtype, LAUNCH))

extern "C" int msau_label_counts(void* stream, const int64_t* labels, int32_t* counts, int B, int64_t hw) {
    MSAU_CHECK_ARG(labels && counts && B > 0 && hw > 0, "label_counts: bad args");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(label_count_kernel, dim3(B), dim3(1024), 0, s, labels, counts, hw);
    MSAU_CHECK_LAUNCH("label_count");
    return 0;
}

extern "C" int msau_label_counts_split(void* stream, const int64_t* labels, int32_t* partial, int B, int64_t hw, int K) {
    MSAU_CHECK_ARG(labels && partial && B > 0 && B <= 65535 && hw > 0 && K >= 1 && K <= 64, "label_counts_split: bad args");
    hipLaunchKernelGGL(label_count_split_kernel, dim3(K, B), dim3(256), 0, static_cast<hipStream_t>(stream), labels, partial, hw, K);
    MSAU_CHECK_LAUNCH("label_count_split");
    return 0;
}

static int ce_blocks(int64_t npix) { return grid_for(npix, 1024); }
extern "C" int64_t msau_ce_ws_floats(int64_t npix_total) { return 2 * ce_blocks(npix_total); }      // (second half: msau_softmax_ce_weighted's weight sums)

// The one-head CE launch of msau_masked_ce, msau_softmax_ce and msau_softmax_ce_weighted (after their own argument checks): the
// register form up to 16 stored channels, the cache form beyond; block partials -> ws[0, nb), with class weights their sums ->
// ws[nb, 2 nb).  `name` labels a launch failure.
template <bool ALL>
static int launch_masked_ce(hipStream_t s, const char* name, int dtype, const void* logits, const int64_t* labels, const int32_t* counts,
                            void* dlogits, float* ws, int nb, int B, int64_t hw, int C, int Cs, float scale, const float* cw) {
#define CE(T, NL, C8) hipLaunchKernelGGL((masked_ce_kernel<T, ALL, C8>), dim3(nb), dim3(kThreads), 0, s, static_cast<const T*>(logits), \
        labels, counts, static_cast<T*>(dlogits), ws, B, hw, C, scale, cw, Cs)
    LOSS_LADDER_16(dtype, false, Cs, CE, LOSS_CACHE(dtype, CE));
#undef CE
    MSAU_CHECK_LAUNCH(name);
    return 0;
}

extern "C" int msau_masked_ce(void* stream, int dtype, const void* logits, const int64_t* labels, const int32_t* counts,
                              void* dlogits, float* loss_accum, float* ws, int B, int64_t hw, int C, int Cs, float scale) {
    MSAU_CHECK_ARG(logits && labels && counts && dlogits && loss_accum && ws, "masked_ce: null pointer");
    MSAU_CHECK_ARG(B > 0 && hw > 0 && C > 0 && C <= Cs && Cs % 8 == 0 && Cs <= 256, "masked_ce: bad dims (n_class <= 256)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = ce_blocks((int64_t)B * hw);
    if (int e = launch_masked_ce<false>(s, "masked_ce", dtype, logits, labels, counts, dlogits, ws, nb, B, hw, C, Cs, scale, nullptr)) return e;
    hipLaunchKernelGGL(ordered_sum_kernel_t<false>, dim3(1), dim3(256), 0, s, ws, nb, loss_accum);
    MSAU_CHECK_LAUNCH("ordered_sum");
    return 0;
}

static int ce_multi_blocks(int64_t npix) { return grid_for(npix, 2048); }
extern "C" int64_t msau_ce_multi_ws_floats(int64_t npix_total) { return ce_multi_blocks(npix_total) + 1; }

extern "C" int msau_masked_ce_multi(void* stream, int dtype, const void* logits, const void* aux, const int64_t* labels,
                                    const int32_t* counts, void* dlogits, void* daux, float* loss, float* ws,
                                    int B, int64_t hw, int C, int Cs, float scale, int counts_k) {
    MSAU_CHECK_ARG(logits && labels && counts && dlogits && loss && ws && (!aux || daux), "masked_ce_multi: null pointer");
    MSAU_CHECK_ARG(counts_k == 1 || (counts_k > 1 && counts_k <= 64 && B <= kCeMaxB), "masked_ce_multi: counts_k > 1 needs B <= 1024");
    MSAU_CHECK_ARG(B > 0 && hw > 0 && C > 0 && C <= Cs && Cs % 8 == 0 && Cs <= 16 && (int64_t)B * hw < (1ll << 31),
                   "masked_ce_multi: bad dims (n_class <= 16, B*H*W < 2^31)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = ce_multi_blocks((int64_t)B * hw);
#define CE_MULTI(T, NL, C8) hipLaunchKernelGGL((masked_ce_multi_kernel<T, NL, C8>), dim3(nb), dim3(kThreads), 0, s, static_cast<const T*>(logits), \
        static_cast<const T*>(aux), labels, counts, static_cast<T*>(dlogits), static_cast<T*>(daux), ws, loss, B, (int)hw, C, scale, counts_k)
    LOSS_LADDER_16(dtype, aux, Cs, CE_MULTI, return msau_set_error(MSAU_ERR_ARG, "masked_ce_multi: no instance for Cs = %d", Cs));
#undef CE_MULTI
    MSAU_CHECK_LAUNCH("masked_ce_multi");
    hipLaunchKernelGGL(ordered_sum_kernel_t<true>, dim3(1), dim3(256), 0, s, ws, nb, loss);
    MSAU_CHECK_LAUNCH("ordered_sum_set");
    return 0;
}

extern "C" int msau_label_hist(void* stream, const int64_t* labels, const int32_t* extent, int32_t* partial, int B, int H, int W,
                               int C, int K) {
    MSAU_CHECK_ARG(labels && partial, "label_hist: null pointer");
    MSAU_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)B * H * W < (1ll << 31) && C > 0 && C <= kHistMaxC && K >= 1 && K <= 64,
                   "label_hist: bad args (B*H*W < 2^31, n_class <= %d, 1 <= K <= 64)", kHistMaxC);
    hipLaunchKernelGGL(label_hist_kernel, dim3(K, B), dim3(256), 0, static_cast<hipStream_t>(stream), labels, extent, partial, H, W, C, K);
    MSAU_CHECK_LAUNCH("label_hist");
    return 0;
}

static int unet_ce_blocks(int64_t npix) { return grid_for(npix, 2048); }
extern "C" int64_t msau_unet_ce_ws_floats(int64_t npix_total) { return 2 * unet_ce_blocks(npix_total); }

// the argument checks of every training entry point of the family, before anything is launched.  `fn` names the entry point.
static int unet_train_check(const char* fn, const void* logits, const void* aux, const int64_t* labels, const int64_t* aux_labels,
                            const float* class_w, const int32_t* hist_partial, int K, const void* dlogits, const void* daux,
                            const float* loss3, const float* ws, int B, int H, int W, int C, int Cs) {
    MSAU_CHECK_ARG(logits && labels && dlogits && loss3 && ws && (!aux || (daux && aux_labels)), "%s: null pointer", fn);
    MSAU_CHECK_ARG(!class_w || (hist_partial && K >= 1 && K <= 64), "%s: class weights need the label histograms (1 <= K <= 64)", fn);
    MSAU_CHECK_ARG(B > 0 && B <= kCeMaxB && H > 0 && W > 0 && (int64_t)B * H * W < (1ll << 31) && C > 0 && C <= Cs && Cs % 8 == 0 && Cs <= 256,
                   "%s: bad dims (B <= %d, B*H*W < 2^31, n_class <= 256)", fn, kCeMaxB);
    return 0;
}

// msau_unet_ce (FOCAL false, gamma unread), the focal loss of msau_unet_cost and (MASKED) both of msau_masked_cost: the same checks,
// the same two launches.  `fn` names the entry point in the messages.
template <bool FOCAL, bool MASKED>
static int unet_ce_run(const char* fn, float gamma, void* stream, int dtype, const void* logits, const void* aux, const int64_t* labels,
                       const int64_t* aux_labels, const int32_t* extent, const float* class_w, const int32_t* hist_partial, int K,
                       void* dlogits, void* daux, float* loss3, float* ws, int B, int H, int W, int C, int Cs) {
    if (int e = unet_train_check(fn, logits, aux, labels, aux_labels, class_w, hist_partial, K, dlogits, daux, loss3, ws, B, H, W, C, Cs)) return e;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = unet_ce_blocks((int64_t)B * H * W);
#define UNET_CE(T, NL, C8) hipLaunchKernelGGL((unet_ce_kernel<T, NL, C8, FOCAL, MASKED>), dim3(nb), dim3(kThreads), 0, s, static_cast<const T*>(logits), \
        static_cast<const T*>(aux), labels, aux_labels, extent, class_w, hist_partial, K, static_cast<T*>(dlogits), static_cast<T*>(daux), \
        ws, B, H, W, C, gamma, Cs)
    LOSS_LADDER_32(dtype, aux, Cs, UNET_CE);
#undef UNET_CE
    MSAU_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(unet_ce_finish_kernel<MASKED>, dim3(1), dim3(256), 0, s, ws, nb, aux ? 1 : 0, loss3);
    MSAU_CHECK_LAUNCH("unet_ce_finish");
    return 0;
}

extern "C" int msau_unet_ce(void* stream, int dtype, const void* logits, const void* aux, const int64_t* labels,
                            const int64_t* aux_labels, const int32_t* extent, const float* class_w, const int32_t* hist_partial, int K,
                            void* dlogits, void* daux, float* loss3, float* ws, int B, int H, int W, int C, int Cs) {
    return unet_ce_run<false, false>("unet_ce", 0.f, stream, dtype, logits, aux, labels, aux_labels, extent, class_w, hist_partial, K, dlogits,
                                     daux, loss3, ws, B, H, W, C, Cs);
}

// the cost of msau_unet_cost / msau_unet_cost_eval / msau_masked_cost / msau_masked_cost_eval: checked before anything else, and
// without a device
static int unet_cost_check(const char* fn, int kind, float param) {
    MSAU_CHECK_ARG(kind == MSAU_COST_CE || kind == MSAU_COST_FOCAL || kind == MSAU_COST_DICE, "%s: unknown cost %d", fn, kind);
    MSAU_CHECK_ARG(kind != MSAU_COST_FOCAL || (param >= 0.f && param < INFINITY), "%s: focal gamma = %g (finite, >= 0)", fn, (double)param);
    MSAU_CHECK_ARG(kind != MSAU_COST_DICE || (param > 0.f && param < INFINITY), "%s: dice smooth = %g (finite, > 0)", fn, (double)param);
    return 0;
}

// the Dice sums of both heads: part[heads][B][K][2][C] written
template <bool MASKED>
static int launch_dice_sums(hipStream_t s, int dtype, const void* logits, const void* aux, const int64_t* labels, const int64_t* aux_labels,
                            const int32_t* extent, float* part, int K, int B, int H, int W, int C, int Cs) {
    const dim3 grid(K, B);
#define DICE_SUMS(T, NL, C8) hipLaunchKernelGGL((unet_dice_sums_kernel<T, NL, C8, MASKED>), grid, dim3(256), 0, s, static_cast<const T*>(logits), \
        static_cast<const T*>(aux), labels, aux_labels, extent, part, B, H, W, C, Cs)
    LOSS_LADDER_32(dtype, aux, Cs, DICE_SUMS);
#undef DICE_SUMS
    MSAU_CHECK_LAUNCH("unet_dice_sums");
    return 0;
}

// Dice training workspace, in floats: [2 B] the documents' losses / B, [2 B C] (hit, miss) pairs, [2 B 64 2 C] the slab rows (K <= 64)
static int64_t dice_tab_at(int B) { return 2 * (int64_t)B; }
static int64_t dice_part_at(int B, int C) { return dice_tab_at(B) + 4 * (int64_t)B * C; }
static int64_t dice_ws_floats(int B, int C) { return dice_part_at(B, C) + 2 * (int64_t)B * 64 * 2 * C; }

extern "C" int64_t msau_unet_cost_ws_floats(int kind, int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    if (kind == MSAU_COST_DICE) return dice_ws_floats(B, C);
    return msau_unet_ce_ws_floats((int64_t)B * H * W);
}

// The Dice loss of msau_unet_cost and (MASKED) of msau_masked_cost, after the cost's own check: the sums, the coefficient step, the
// finish launch and the gradient pass.  MASKED: hist_partial is the one label map's.
template <bool MASKED>
static int unet_dice_run(const char* fn, float eps, void* stream, int dtype, const void* logits, const void* aux, const int64_t* labels,
                         const int64_t* aux_labels, const int32_t* extent, const float* class_w, const int32_t* hist_partial, int K,
                         void* dlogits, void* daux, float* loss3, float* ws, int B, int H, int W, int C, int Cs) {
    if (int e = unet_train_check(fn, logits, aux, labels, aux_labels, class_w, hist_partial, K, dlogits, daux, loss3, ws, B, H, W, C, Cs)) return e;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nl = aux ? 2 : 1;
    float* part = ws + dice_part_at(B, C);
    float2* tab = reinterpret_cast<float2*>(ws + dice_tab_at(B));
    if (int e = launch_dice_sums<MASKED>(s, dtype, logits, aux, labels, aux_labels, extent, part, K, B, H, W, C, Cs)) return e;
    // the documents' losses / B of head t -> ws[t * B + b]: unet_ce_finish_kernel then adds each head's B values as it adds block partials
    hipLaunchKernelGGL(unet_dice_coef_kernel<MASKED>, dim3(B, nl), dim3(256), 0, s, part, K, hist_partial, K, class_w, eps, tab, ws, 1, B,
                       1.f / (float)B, B, C);
    MSAU_CHECK_LAUNCH("unet_dice_coef");
    hipLaunchKernelGGL(unet_ce_finish_kernel<MASKED>, dim3(1), dim3(256), 0, s, ws, B, aux ? 1 : 0, loss3);
    MSAU_CHECK_LAUNCH("unet_ce_finish");
    const int nb = unet_ce_blocks((int64_t)B * H * W);
#define DICE_GRAD(T, NL, C8) hipLaunchKernelGGL((unet_dice_grad_kernel<T, NL, C8, MASKED>), dim3(nb), dim3(kThreads), 0, s, static_cast<const T*>(logits), \
        static_cast<const T*>(aux), labels, aux_labels, extent, tab, static_cast<T*>(dlogits), static_cast<T*>(daux), B, H, W, C, Cs)
    LOSS_LADDER_32(dtype, aux, Cs, DICE_GRAD);
#undef DICE_GRAD
    MSAU_CHECK_LAUNCH("unet_dice_grad");
    return 0;
}

extern "C" int msau_unet_cost(void* stream, int dtype, int kind, float param, const void* logits, const void* aux, const int64_t* labels,
                              const int64_t* aux_labels, const int32_t* extent, const float* class_w, const int32_t* hist_partial, int K,
                              void* dlogits, void* daux, float* loss3, float* ws, int B, int H, int W, int C, int Cs) {
    if (int e = unet_cost_check("unet_cost", kind, param)) return e;
    MSAU_CHECK_ARG(kind != MSAU_COST_DICE || (hist_partial && K >= 1 && K <= 64), "unet_cost: dice needs the label histograms (1 <= K <= 64)");
    if (kind == MSAU_COST_CE)
        return msau_unet_ce(stream, dtype, logits, aux, labels, aux_labels, extent, class_w, hist_partial, K, dlogits, daux, loss3, ws, B, H, W, C, Cs);
    if (kind == MSAU_COST_FOCAL)
        return unet_ce_run<true, false>("unet_cost", param, stream, dtype, logits, aux, labels, aux_labels, extent, class_w, hist_partial, K,
                                        dlogits, daux, loss3, ws, B, H, W, C, Cs);
    return unet_dice_run<false>("unet_cost", param, stream, dtype, logits, aux, labels, aux_labels, extent, class_w, hist_partial, K, dlogits,
                                daux, loss3, ws, B, H, W, C, Cs);
}

// The masked cost: the loss of TrainEngine.step / MSAUWrapper.loss under a cost and class weights.  Both heads are
// scored against ONE label map over the pixels with a label in [1, C), head weights 1 and 1.  The cross entropy and the focal loss
// without class weights need only the documents' numbers of labelled pixels: when no histogram is given, this call takes one itself,
// kMaskedHistK rows per document, into the tail of its workspace.
constexpr int kMaskedHistK = 16;

extern "C" int64_t msau_masked_cost_ws_floats(int kind, int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    if (kind == MSAU_COST_DICE) return dice_ws_floats(B, C);
    return msau_unet_ce_ws_floats((int64_t)B * H * W) + (int64_t)B * kMaskedHistK * C;
}

extern "C" int msau_masked_cost(void* stream, int dtype, int kind, float param, const void* logits, const void* aux, const int64_t* labels,
                                const int32_t* extent, const float* class_w, const int32_t* hist_partial, int K, void* dlogits, void* daux,
                                float* loss3, float* ws, int B, int H, int W, int C, int Cs) {
    if (int e = unet_cost_check("masked_cost", kind, param)) return e;
    MSAU_CHECK_ARG(kind != MSAU_COST_DICE || (hist_partial && K >= 1 && K <= 64), "masked_cost: dice needs the label histograms (1 <= K <= 64)");
    MSAU_CHECK_ARG(!hist_partial || (K >= 1 && K <= 64), "masked_cost: K = %d rows of the label histograms (1 <= K <= 64)", K);
    if (kind == MSAU_COST_DICE)
        return unet_dice_run<true>("masked_cost", param, stream, dtype, logits, aux, labels, labels, extent, class_w, hist_partial, K, dlogits,
                                   daux, loss3, ws, B, H, W, C, Cs);
    if (!hist_partial) {
        if (int e = unet_train_check("masked_cost", logits, aux, labels, labels, class_w, hist_partial, K, dlogits, daux, loss3, ws, B, H, W, C, Cs)) return e;
        MSAU_CHECK_ARG(C <= kHistMaxC, "masked_cost: n_class <= %d", kHistMaxC);
        int32_t* own = reinterpret_cast<int32_t*>(ws + msau_unet_ce_ws_floats((int64_t)B * H * W));
        if (int e = msau_label_hist(stream, labels, extent, own, B, H, W, C, kMaskedHistK)) return e;
        hist_partial = own;
        K = kMaskedHistK;
    }
    if (kind == MSAU_COST_FOCAL)
        return unet_ce_run<true, true>("masked_cost", param, stream, dtype, logits, aux, labels, labels, extent, class_w, hist_partial, K, dlogits,
                                       daux, loss3, ws, B, H, W, C, Cs);
    return unet_ce_run<false, true>("masked_cost", 0.f, stream, dtype, logits, aux, labels, labels, extent, class_w, hist_partial, K, dlogits,
                                    daux, loss3, ws, B, H, W, C, Cs);
}

extern "C" int64_t msau_unet_eval_ws_bytes(int B, int K) {
    return B > 0 && K > 0 ? (int64_t)B * K * (int64_t)sizeof(UnetEvalRow) : 0;
}

// msau_unet_eval (FOCAL false, gamma unread), the focal rows of msau_unet_cost_eval and (MASKED) the rows of msau_masked_cost_eval
template <bool FOCAL, bool MASKED>
static int unet_eval_run(const char* fn, float gamma, void* stream, int dtype, const void* logits, const void* aux, const int64_t* labels,
                         const int64_t* aux_labels, const int32_t* extent, const float* class_w, int K, float* doc_loss,
                         int32_t* doc_counts, void* ws, int B, int H, int W, int C, int Cs) {
    MSAU_CHECK_ARG(logits && labels && doc_loss && doc_counts && ws && (!aux || aux_labels), "%s: null pointer", fn);
    MSAU_CHECK_ARG(K >= 1 && K <= 256, "%s: K = %d workgroups per document (1 <= K <= 256)", fn, K);
    MSAU_CHECK_ARG(B > 0 && B <= kCeMaxB && H > 0 && W > 0 && (int64_t)B * H * W < (1ll << 31) && C > 0 && C <= Cs && Cs % 8 == 0 && Cs <= 256,
                   "%s: bad dims (B <= %d, B*H*W < 2^31, n_class <= 256)", fn, kCeMaxB);
    hipStream_t s = static_cast<hipStream_t>(stream);
    UnetEvalRow* rows = static_cast<UnetEvalRow*>(ws);
    const dim3 grid(K, B);
#define UNET_EVAL(T, NL, C8) hipLaunchKernelGGL((unet_eval_kernel<T, NL, C8, FOCAL, MASKED>), grid, dim3(256), 0, s, static_cast<const T*>(logits), \
        static_cast<const T*>(aux), labels, aux_labels, extent, class_w, rows, H, W, C, gamma, Cs)
    LOSS_LADDER_32(dtype, aux, Cs, UNET_EVAL);
#undef UNET_EVAL
    MSAU_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(unet_eval_finish_kernel, dim3((2 * B + 255) / 256), dim3(256), 0, s, rows, B, K, doc_loss, doc_counts);
    MSAU_CHECK_LAUNCH("unet_eval_finish");
    return 0;
}

extern "C" int msau_unet_eval(void* stream, int dtype, const void* logits, const void* aux, const int64_t* labels,
                              const int64_t* aux_labels, const int32_t* extent, const float* class_w, int K, float* doc_loss,
                              int32_t* doc_counts, void* ws, int B, int H, int W, int C, int Cs) {
    return unet_eval_run<false, false>("unet_eval", 0.f, stream, dtype, logits, aux, labels, aux_labels, extent, class_w, K, doc_loss, doc_counts,
                                       ws, B, H, W, C, Cs);
}

// Dice evaluation workspace, in bytes: msau_unet_eval's rows, then [2 B K 2 C] floats of slab rows, then [heads B min(K, 64) C] int32
// of label histograms (heads: 2 label maps under UNetLoss, 1 under the masked cost)
static int dice_eval_kh(int K) { return K < 64 ? K : 64; }
static int64_t cost_eval_ws_bytes(int kind, int B, int K, int C, int maps) {
    const int64_t rows = msau_unet_eval_ws_bytes(B, K);
    if (kind != MSAU_COST_DICE || rows == 0 || C <= 0) return rows;
    return rows + 4 * (2 * (int64_t)B * K * 2 * C + maps * (int64_t)B * dice_eval_kh(K) * C);
}
extern "C" int64_t msau_unet_cost_eval_ws_bytes(int kind, int B, int K, int C) { return cost_eval_ws_bytes(kind, B, K, C, 2); }
extern "C" int64_t msau_masked_cost_eval_ws_bytes(int kind, int B, int K, int C) { return cost_eval_ws_bytes(kind, B, K, C, 1); }

// msau_unet_cost_eval and (MASKED: aux_labels = labels) msau_masked_cost_eval
template <bool MASKED>
static int unet_cost_eval_run(const char* fn, void* stream, int dtype, int kind, float param, const void* logits, const void* aux,
                              const int64_t* labels, const int64_t* aux_labels, const int32_t* extent, const float* class_w, int K,
                              float* doc_loss, int32_t* doc_counts, void* ws, int B, int H, int W, int C, int Cs) {
    if (int e = unet_cost_check(fn, kind, param)) return e;
    if (kind == MSAU_COST_FOCAL)
        return unet_eval_run<true, MASKED>(fn, param, stream, dtype, logits, aux, labels, aux_labels, extent, class_w, K, doc_loss,
                                           doc_counts, ws, B, H, W, C, Cs);
    // the counts (and, for the cross entropy, the losses) are msau_unet_eval's own
    if (int e = unet_eval_run<false, MASKED>(MASKED ? fn : "unet_eval", 0.f, stream, dtype, logits, aux, labels, aux_labels, extent, class_w, K,
                                             doc_loss, doc_counts, ws, B, H, W, C, Cs)) return e;
    if (kind == MSAU_COST_CE) return 0;
    // Dice: the sums over the same K slabs, the label histograms taken here, and the coefficient step writes doc_loss[b][t] over the
    // cross entropy's (head 1 of a one-head call keeps msau_unet_eval's 0)
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nl = aux ? 2 : 1, Kh = dice_eval_kh(K);
    float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + msau_unet_eval_ws_bytes(B, K));
    int32_t* hist = reinterpret_cast<int32_t*>(part + 2 * (int64_t)B * K * 2 * C);
    for (int t = 0; t < (MASKED ? 1 : nl); ++t)
        if (int e = msau_label_hist(stream, t ? aux_labels : labels, extent, hist + (int64_t)t * B * Kh * C, B, H, W, C, Kh)) return e;
    if (int e = launch_dice_sums<MASKED>(s, dtype, logits, aux, labels, aux_labels, extent, part, K, B, H, W, C, Cs)) return e;
    hipLaunchKernelGGL(unet_dice_coef_kernel<MASKED>, dim3(B, nl), dim3(256), 0, s, part, K, hist, Kh, class_w, param,
                       static_cast<float2*>(nullptr), doc_loss, 2, 1, 1.f, B, C);
    MSAU_CHECK_LAUNCH("unet_dice_coef");
    return 0;
}

extern "C" int msau_unet_cost_eval(void* stream, int dtype, int kind, float param, const void* logits, const void* aux,
                                   const int64_t* labels, const int64_t* aux_labels, const int32_t* extent, const float* class_w, int K,
                                   float* doc_loss, int32_t* doc_counts, void* ws, int B, int H, int W, int C, int Cs) {
    return unet_cost_eval_run<false>("unet_cost_eval", stream, dtype, kind, param, logits, aux, labels, aux_labels, extent, class_w, K, doc_loss,
                                     doc_counts, ws, B, H, W, C, Cs);
}

extern "C" int msau_masked_cost_eval(void* stream, int dtype, int kind, float param, const void* logits, const void* aux,
                                     const int64_t* labels, const int32_t* extent, const float* class_w, int K, float* doc_loss,
                                     int32_t* doc_counts, void* ws, int B, int H, int W, int C, int Cs) {
    return unet_cost_eval_run<true>("masked_cost_eval", stream, dtype, kind, param, logits, aux, labels, labels, extent, class_w, K, doc_loss,
                                    doc_counts, ws, B, H, W, C, Cs);
}

extern "C" int msau_softmax_ce(void* stream, int dtype, const void* logits, const int64_t* labels, void* dlogits,
                               float* loss_accum, float* ws, int B, int64_t hw, int C, int Cs, float scale) {
    MSAU_CHECK_ARG(logits && labels && dlogits && loss_accum && ws, "softmax_ce: null pointer");
    MSAU_CHECK_ARG(B > 0 && hw > 0 && C > 0 && C <= Cs && Cs % 8 == 0 && Cs <= 256, "softmax_ce: bad dims (n_class <= 256)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = ce_blocks((int64_t)B * hw);
    if (int e = launch_masked_ce<true>(s, "softmax_ce", dtype, logits, labels, nullptr, dlogits, ws, nb, B, hw, C, Cs, scale, nullptr)) return e;
    hipLaunchKernelGGL(ordered_sum_kernel_t<false>, dim3(1), dim3(256), 0, s, ws, nb, loss_accum);
    MSAU_CHECK_LAUNCH("ordered_sum");
    return 0;
}

extern "C" int msau_softmax_ce_weighted(void* stream, int dtype, const void* logits, const int64_t* labels, const float* class_w,
                                        void* dlogits, float* sums, float* ws, int B, int64_t hw, int C, int Cs) {
    MSAU_CHECK_ARG(logits && labels && class_w && dlogits && sums && ws, "softmax_ce_weighted: null pointer");
    MSAU_CHECK_ARG(B > 0 && hw > 0 && C > 0 && C <= Cs && Cs % 8 == 0 && Cs <= 256, "softmax_ce_weighted: bad dims (n_class <= 256)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = ce_blocks((int64_t)B * hw);
    if (int e = launch_masked_ce<true>(s, "softmax_ce_weighted", dtype, logits, labels, nullptr, dlogits, ws, nb, B, hw, C, Cs, 1.f, class_w)) return e;
    hipLaunchKernelGGL(ordered_sum_kernel_t<false>, dim3(1), dim3(256), 0, s, ws, nb, sums);
    hipLaunchKernelGGL(ordered_sum_kernel_t<false>, dim3(1), dim3(256), 0, s, ws + nb, nb, sums + 1);
    MSAU_CHECK_LAUNCH("ordered_sum");
    return 0;
}

extern "C" int msau_eval_confusion(void* stream, int dtype, const void* logits, const int64_t* labels, int64_t* counts, int B, int H,
                                   int W, int C, int Cs, int zero_as, const int32_t* extent) {
    MSAU_CHECK_ARG(logits && labels && counts && B > 0 && H > 0 && W > 0, "eval_confusion: bad args");
    MSAU_CHECK_ARG(C >= 1 && C <= kConfusionMaxC && C <= Cs && Cs % 8 == 0, "eval_confusion: C = %d (Cs = %d) must satisfy 1 <= C <= %d, C <= Cs, Cs %% 8 == 0",
                   C, Cs, kConfusionMaxC);
    MSAU_CHECK_ARG(zero_as < C, "eval_confusion: zero_as = %d is not a class of %d", zero_as, C);
    const int64_t npix = (int64_t)B * H * W;
    MSAU_CHECK_ARG(npix < (1ll << 40), "eval_confusion: too many pixels");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // at least 4 pixels per lane and at most 512 workgroups: the LDS histogram's clear and flush stay small beside the pixels
    const dim3 grid(grid_for(cdiv64(npix, 4), 512));
    unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
    DISPATCH_T(dtype,
               hipLaunchKernelGGL(eval_confusion_kernel<float>, grid, dim3(kThreads), 0, s, static_cast<const float*>(logits), labels, out, npix, H, W, C, Cs, zero_as, extent),
               hipLaunchKernelGGL(eval_confusion_kernel<bf16_t>, grid, dim3(kThreads), 0, s, static_cast<const bf16_t*>(logits), labels, out, npix, H, W, C, Cs, zero_as, extent));
    MSAU_CHECK_LAUNCH("eval_confusion");
    return 0;
}

extern "C" int msau_softmax_channels_nchw(void* stream, const float* logits, float* pred, int B, int C, int64_t hw) {
    MSAU_CHECK_ARG(logits && pred && B > 0 && C > 0 && hw > 0, "softmax: bad args");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(softmax_nchw_kernel, dim3(grid_for((int64_t)B * hw)), dim3(kThreads), 0, s, logits, pred, B, C, hw);
    MSAU_CHECK_LAUNCH("softmax_nchw");
    return 0;
}

extern "C" int msau_softmax_argmax_nhwc(void* stream, int dtype, const void* logits, float* probs, uint8_t* argmax,
                                        int64_t npix, int C, int Cs) {
    MSAU_CHECK_ARG(logits && probs && argmax && npix > 0 && C > 0 && C <= 255 && C <= Cs, "softmax_argmax: bad args");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DISPATCH_T(dtype,
               hipLaunchKernelGGL(softmax_argmax_nhwc_kernel<float>, dim3(grid_for(npix)), dim3(kThreads), 0, s, static_cast<const float*>(logits), probs, argmax, npix, C, Cs),
               hipLaunchKernelGGL(softmax_argmax_nhwc_kernel<bf16_t>, dim3(grid_for(npix)), dim3(kThreads), 0, s, static_cast<const bf16_t*>(logits), probs, argmax, npix, C, Cs));
    MSAU_CHECK_LAUNCH("softmax_argmax_nhwc");
    return 0;
}
