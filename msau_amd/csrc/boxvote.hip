// Entity-level predictions by box vote (FUNSD evaluation over entities or words instead of pixels): for every box of a list the
// histogram of the per-pixel classes of its voting pixels, the winning class and, per (box value, winner), one count of an int64
// matrix.  The per-pixel class is the one msau_eval_confusion counts: the first maximum of the C stored logits as float, NaN
// counting as the maximum, 0 -> zero_as when zero_as >= 0.  A box is clipped as raster_owner_kernel / raster_owner_ext_kernel clip
// it; with an owner map (the one those kernels wrote for THIS list) only the pixels the box owns vote, so every pixel votes once.
//
// Who takes a box.  A workgroup of four waves takes the four consecutive boxes [4g, 4g + 4), groups in a grid-stride loop:
//   - wave k alone takes box 4g + k when its clipped area is at most BV_WAVE_AREA = 256 pixels (at most four trips of 64 pixels):
//     no LDS and no barrier, and the four small boxes of a group run side by side.  Text lines and words of a chargrid are of this
//     size, so this is the common path.
//   - a larger box is taken by all four waves, wave k the pixels [64 k, 64 k + 64) of every 256; the waves' class counts are
//     merged through LDS and wave 0 writes the result.
// Counting takes no atomics: with C <= 64, lane c of a wave holds class c's count; per trip of 64 pixels one ballot and one
// population count per class.  The winner is the largest (count, -class) over the lanes: the smallest class among the most frequent.
// Everything is an integer and every element of pred / votes / hist is written exactly once; the one global atomic is the 64-bit
// add per counted box into `counts`.
//
// With -DMSAU_BOXVOTE_CPU the file compiles as plain C++: the same clipping, pixel classification and summary, the lanes of a wave
// one after another (tests/test_box_vote_cpu.py builds that form with the host compiler).
#ifdef MSAU_BOXVOTE_CPU
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/msau_hip.h"
#define BV_DEV static inline
struct bv_bf16 { uint16_t bits; };
BV_DEV float bv_f32(float v) { return v; }
BV_DEV float bv_f32(bv_bf16 v) { uint32_t u = (uint32_t)v.bits << 16; float f; memcpy(&f, &u, 4); return f; }   // exact
static inline int bv_min(int a, int b) { return a < b ? a : b; }
static inline int bv_max(int a, int b) { return a > b ? a : b; }
#else
#include "msau_common.h"
#define BV_DEV __device__ __forceinline__
#define bv_min min
#define bv_max max
#endif

#define BV_MAXC 64            // classes: lane c of a wave64 counts class c (the limit of msau_eval_confusion)
#define BV_WAVES 4            // waves of a workgroup = boxes of a group
#define BV_WAVE_AREA 256      // a box of at most this many clipped pixels is one wave's, a larger one the workgroup's
#define BV_GRID_CAP 1024     // workgroups, i.e. 4096 boxes per sweep of the grid-stride loop (raster_owner: 4096 boxes)

struct BvBox { int b, y0, x0, w, area; };   // area 0: nothing votes

struct BvArgs {
    const void* logits;
    const int32_t* boxes;
    const int32_t* owner;
    const int32_t* extent;
    int32_t* pred;
    int32_t* votes;
    int32_t* hist;
    unsigned long long* counts;
    int n, B, H, W, C, Cs, zero_as;
};

// strictly greater: the first maximum wins; a NaN counts as the maximum, as in torch.argmax (first_max of loss.hip)
BV_DEV void bv_first_max(float v, int c, float& bv, int& best) {
    if (v > bv || (v != v && bv == bv)) { bv = v; best = c; }
}

// the clipping of raster_owner_kernel (extent == NULL) / raster_owner_ext_kernel
BV_DEV BvBox bv_clip(const BvArgs& a, int i) {
    const int32_t* bx = a.boxes + (size_t)i * 6;
    BvBox r = {bx[0], 0, 0, 0, 0};
    if (r.b < 0 || r.b >= a.B) return r;
    int eh = a.H, ew = a.W;
    if (a.extent) { eh = bv_min(bv_max(a.extent[2 * r.b], 0), a.H); ew = bv_min(bv_max(a.extent[2 * r.b + 1], 0), a.W); }
    const int y0 = bv_max(bx[1], 0), y1 = bv_min(bx[2], eh), x0 = bv_max(bx[3], 0), x1 = bv_min(bx[4], ew);
    if (y1 <= y0 || x1 <= x0) return r;
    r.y0 = y0; r.x0 = x0; r.w = x1 - x0; r.area = r.w * (y1 - y0);
    return r;
}

// the class pixel t (< area) of box i votes for, -1 when it does not vote
template <typename T>
BV_DEV int bv_vote(const BvArgs& a, const BvBox& bx, int i, int t) {
    const int y = bx.y0 + t / bx.w, x = bx.x0 + t % bx.w;
    const size_t p = ((size_t)bx.b * a.H + y) * a.W + x;
    if (a.owner && a.owner[p] != i) return -1;
    const T* l = static_cast<const T*>(a.logits) + p * a.Cs;
    int best = 0;
    float bv = -INFINITY;
    for (int c0 = 0; c0 < a.C; c0 += 8) {
#ifdef MSAU_BOXVOTE_CPU
        for (int j = 0; j < 8; ++j)
            if (c0 + j < a.C) bv_first_max(bv_f32(l[c0 + j]), c0 + j, bv, best);
#else
        const typename Vec8<T>::type v8 = load8<T>(l + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c0 + j < a.C) bv_first_max((float)v8[j], c0 + j, bv, best);
#endif
    }
    if (best == 0 && a.zero_as >= 0) best = a.zero_as;
    return best;
}

// (count, class) as one ordered key: the larger count wins, among equal counts the smaller class
BV_DEV long long bv_key(int cnt, int c) { return ((long long)cnt << 6) | (long long)(BV_MAXC - 1 - c); }

// box i's summary from the winning key and the number of voting pixels (one lane)
BV_DEV void bv_finish(const BvArgs& a, int i, long long key, int total) {
    const int win = total > 0 ? BV_MAXC - 1 - (int)(key & (BV_MAXC - 1)) : -1;
    a.pred[i] = win;
    a.votes[2 * (size_t)i] = total > 0 ? (int)(key >> 6) : 0;
    a.votes[2 * (size_t)i + 1] = total;
    const int v = a.boxes[(size_t)i * 6 + 5];
    if (a.counts && win >= 0 && v >= 1 && v < a.C) {
#ifdef MSAU_BOXVOTE_CPU
        a.counts[(size_t)v * a.C + win] += 1ull;
#else
        atomicAdd(a.counts + (size_t)v * a.C + win, 1ull);
#endif
    }
}

// the argument checks both forms share -> a message, or NULL when the call is fine
static const char* bv_bad_args(int dtype, const void* logits, const int32_t* boxes, int n, const int32_t* pred, const int32_t* votes,
                               int B, int H, int W, int C, int Cs, int zero_as, char* msg, size_t len) {
    if (dtype != MSAU_F32 && dtype != MSAU_BF16) { snprintf(msg, len, "bad dtype %d", dtype); return msg; }
    if (n < 0 || B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31)) {
        snprintf(msg, len, "bad shape n = %d, B = %d, H = %d, W = %d", n, B, H, W);
        return msg;
    }
    if (C < 1 || C > BV_MAXC || C > Cs || Cs % 8 != 0) {
        snprintf(msg, len, "C = %d (Cs = %d) must satisfy 1 <= C <= %d, C <= Cs, Cs %% 8 == 0", C, Cs, BV_MAXC);
        return msg;
    }
    if (zero_as >= C) { snprintf(msg, len, "zero_as = %d is not a class of %d", zero_as, C); return msg; }
    if (n > 0 && !(logits && boxes && pred && votes)) { snprintf(msg, len, "null logits / boxes / pred / votes with n = %d", n); return msg; }
    return 0;
}

#ifdef MSAU_BOXVOTE_CPU
namespace {
// one trip of a wave, lane by lane: the votes of pixels [t0, t0 + 64) into cnt[class] (the ballot + population count per class)
template <typename T>
void bv_trip_cpu(const BvArgs& a, const BvBox& bx, int i, int64_t t0, int* cnt) {
    int cls[64];
    for (int lane = 0; lane < 64; ++lane) cls[lane] = t0 + lane < bx.area ? bv_vote<T>(a, bx, i, (int)(t0 + lane)) : -1;
    for (int lane = 0; lane < a.C; ++lane)
        for (int l = 0; l < 64; ++l) cnt[lane] += cls[l] == lane;
}
// the wave's reduction and wave 0's writes
void bv_write_cpu(const BvArgs& a, int i, const int* cnt) {
    long long key = -1;
    int total = 0;
    for (int lane = 0; lane < a.C; ++lane) {
        if (a.hist) a.hist[(size_t)i * a.C + lane] = cnt[lane];
        const long long k = bv_key(cnt[lane], lane);
        key = k > key ? k : key;
        total += cnt[lane];
    }
    bv_finish(a, i, key, total);
}
template <typename T>
void bv_run_cpu(const BvArgs& a) {
    const int ngroups = (a.n + BV_WAVES - 1) / BV_WAVES;
    for (int g = 0; g < ngroups; ++g) {
        for (int wave = 0; wave < BV_WAVES; ++wave) {                      // a wave's own small box
            const int i = g * BV_WAVES + wave;
            if (i >= a.n) continue;
            const BvBox bx = bv_clip(a, i);
            if (bx.area > BV_WAVE_AREA) continue;
            int cnt[64] = {0};
            for (int64_t t0 = 0; t0 < bx.area; t0 += 64) bv_trip_cpu<T>(a, bx, i, t0, cnt);
            bv_write_cpu(a, i, cnt);
        }
        for (int k = 0; k < BV_WAVES; ++k) {                               // the group's large boxes, all waves on each
            const int i = g * BV_WAVES + k;
            if (i >= a.n) break;
            const BvBox bx = bv_clip(a, i);
            if (bx.area <= BV_WAVE_AREA) continue;
            int lds[BV_WAVES][64];
            memset(lds, 0, sizeof(lds));
            for (int wave = 0; wave < BV_WAVES; ++wave)
                for (int64_t t0 = 64 * wave; t0 < bx.area; t0 += 64 * BV_WAVES) bv_trip_cpu<T>(a, bx, i, t0, lds[wave]);
            int cnt[64];
            for (int lane = 0; lane < 64; ++lane) cnt[lane] = lds[0][lane] + lds[1][lane] + lds[2][lane] + lds[3][lane];
            bv_write_cpu(a, i, cnt);
        }
    }
}
}  // namespace

// the launch, lane by lane on the host: the arguments of msau_box_vote without the stream; the message of a refused call goes to
// `msg` (at least 160 bytes, may be NULL)
extern "C" int msau_box_vote_cpu(int dtype, const void* logits, const int32_t* boxes, int n, const int32_t* owner, int32_t* pred,
                                 int32_t* votes, int32_t* hist, int64_t* counts, int B, int H, int W, int C, int Cs, int zero_as,
                                 const int32_t* extent, char* msg) {
    char buf[144];
    if (bv_bad_args(dtype, logits, boxes, n, pred, votes, B, H, W, C, Cs, zero_as, buf, sizeof(buf))) {
        if (msg) snprintf(msg, 160, "box_vote: %s", buf);
        return MSAU_ERR_ARG;
    }
    if (n == 0) return 0;
    const BvArgs a = {logits, boxes, owner, extent, pred, votes, hist, reinterpret_cast<unsigned long long*>(counts), n, B, H, W, C, Cs, zero_as};
    if (dtype == MSAU_F32) bv_run_cpu<float>(a);
    else bv_run_cpu<bv_bf16>(a);
    return 0;
}
#else
namespace {

// the votes of one trip (every lane its pixel's class, -1 = none) into the lanes' counts: lane c counts class c
__device__ __forceinline__ int bv_count(int cls, int cnt, int C, int lane) {
    for (int c = 0; c < C; ++c) {
        const unsigned long long m = __ballot(cls == c);
        if (lane == c) cnt += __popcll(m);
    }
    return cnt;
}

// lane c holds class c's count of box i (0 for c >= C): histogram, winner and total, written by this wave
__device__ __forceinline__ void bv_write(const BvArgs& a, int i, int cnt, int lane) {
    if (a.hist && lane < a.C) a.hist[(size_t)i * a.C + lane] = cnt;
    long long key = lane < a.C ? bv_key(cnt, lane) : -1;
    int total = cnt;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const long long ok = __shfl_xor(key, s, 64);
        key = ok > key ? ok : key;
        total += __shfl_xor(total, s, 64);
    }
    if (lane == 0) bv_finish(a, i, key, total);
}

template <typename T>
__global__ __launch_bounds__(64 * BV_WAVES) void box_vote_kernel(const BvArgs a) {
    __shared__ int merge[BV_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ngroups = (a.n + BV_WAVES - 1) / BV_WAVES;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int i = g * BV_WAVES + wave;                                 // this wave's own box
        if (i < a.n) {
            const BvBox bx = bv_clip(a, i);
            if (bx.area <= BV_WAVE_AREA) {
                int cnt = 0;
                for (int t0 = 0; t0 < bx.area; t0 += 64) {
                    const int t = t0 + lane;
                    cnt = bv_count(t < bx.area ? bv_vote<T>(a, bx, i, t) : -1, cnt, a.C, lane);
                }
                bv_write(a, i, cnt, lane);
            }
        }
        for (int k = 0; k < BV_WAVES; ++k) {                               // the group's large boxes: every condition is uniform
            const int j = g * BV_WAVES + k;                                // over the workgroup, so are the barriers
            if (j >= a.n) break;
            const BvBox bx = bv_clip(a, j);
            if (bx.area <= BV_WAVE_AREA) continue;
            int cnt = 0;
            for (int64_t t0 = 64 * wave; t0 < bx.area; t0 += 64 * BV_WAVES) {
                const int64_t t = t0 + lane;
                cnt = bv_count(t < bx.area ? bv_vote<T>(a, bx, j, (int)t) : -1, cnt, a.C, lane);
            }
            merge[wave][lane] = cnt;
            __syncthreads();
            if (wave == 0) {
                cnt = 0;
#pragma unroll
                for (int w = 0; w < BV_WAVES; ++w) cnt += merge[w][lane];
                bv_write(a, j, cnt, lane);
            }
            __syncthreads();                                               // wave 0 has read `merge` before the next box fills it
        }
    }
}

}  // namespace

extern "C" int msau_box_vote(void* stream, int dtype, const void* logits, const int32_t* boxes, int n, const int32_t* owner,
                             int32_t* pred, int32_t* votes, int32_t* hist, int64_t* counts, int B, int H, int W, int C, int Cs,
                             int zero_as, const int32_t* extent) {
    char buf[160];
    const char* bad = bv_bad_args(dtype, logits, boxes, n, pred, votes, B, H, W, C, Cs, zero_as, buf, sizeof(buf));
    MSAU_CHECK_ARG(!bad, "box_vote: %s", bad);
    if (n == 0) return 0;
    const BvArgs a = {logits, boxes, owner, extent, pred, votes, hist, reinterpret_cast<unsigned long long*>(counts), n, B, H, W, C, Cs, zero_as};
    const int ngroups = (n + BV_WAVES - 1) / BV_WAVES;
    const dim3 grid(ngroups < BV_GRID_CAP ? ngroups : BV_GRID_CAP);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == MSAU_F32) hipLaunchKernelGGL(box_vote_kernel<float>, grid, dim3(64 * BV_WAVES), 0, s, a);
    else hipLaunchKernelGGL(box_vote_kernel<bf16_t>, grid, dim3(64 * BV_WAVES), 0, s, a);
    MSAU_CHECK_LAUNCH("box_vote");
    return 0;
}
#endif
