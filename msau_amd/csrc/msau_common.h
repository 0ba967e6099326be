// Internal helpers shared by the kernels of libmsau_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/msau_hip.h"

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

#define MSAU_LDS_LIMIT (160 * 1024)

int msau_set_error(int code, const char* fmt, ...);

// ---- msau_conv_pair (pair_route in conv_pair.hip picks the family and the instance; DESIGN.md, "conv_pair routing")
// The two flag combinations the kernels are compiled for: the residual block's forward, and its data gradient ...
constexpr int kFwd1 = MSAU_PAIR_RELU_IN | MSAU_PAIR_RELU_MID, kFwd2 = MSAU_CONV_ADD | MSAU_CONV_RELU_OUT;
constexpr int kBwd1 = MSAU_PAIR_MASK_MID, kBwd2 = MSAU_CONV_MASK_A | MSAU_CONV_ADD;
// ... and the rider flags of flags1, which do not change the direction: a rider belongs to one direction (MSAU_PAIR_TILES to both)
constexpr int kPairFwdRiders = MSAU_PAIR_COUPLE, kPairBwdRiders = MSAU_PAIR_LRN_BWD | MSAU_PAIR_WGRAD1 | MSAU_PAIR_DCOUPLE;
constexpr int kPairRiders = MSAU_PAIR_TILES | kPairFwdRiders | kPairBwdRiders;
enum { PAIR_NONE = 0, PAIR_TILE = 1, PAIR_ROWS = 2 };      // the families (= the answers of msau_conv_pair_instance)
enum { PAIR_FWD = 1, PAIR_BWD = 2 };
// the direction of a descriptor, 0 = neither flag set or a rider of the other direction; MSAU_CONV_POOL rides on the forward
static inline int msau_pair_direction(const msau_conv_pair_desc* d) {
    const int f1 = d->flags1 & ~kPairRiders;
    if (f1 == kFwd1 && (d->flags2 & ~MSAU_CONV_POOL) == kFwd2 && !(d->flags1 & kPairBwdRiders)) return PAIR_FWD;
    if (f1 == kBwd1 && d->flags2 == kBwd2 && !(d->flags1 & kPairFwdRiders)) return PAIR_BWD;
    return 0;
}
struct PairRoute {
    int family, dir, inst;                       // PAIR_*, PAIR_FWD / PAIR_BWD, the instance's number in its family's table (0 = none)
    int tw, tiles_x, tiles_y;                    // tile family: tile width (16 tw - 2 output columns) and tiles per image
    int nstrips, SH, nseg, ntasks, workgroups;   // row family: strips, segment height, segments per strip, tasks, grid
    int64_t plane_bytes;                         // bytes of one ReLU-mask plane in the layout of the instance (no instance: the tile kernels')
    int slabs;                                   // MSAU_PAIR_WGRAD1: the slabs the launch writes, 0 = the flag is not set
};
// conv_rows.hip: the row-streaming instances for 8 and 16 channels, bf16.  The contract of msau_conv2d's families below: _case is
// the number of the instance that runs the descriptor (0 = none; for a descriptor behind pair_route's own checks: direction, operands
// every family needs), _launch launches exactly that instance, _split is its task split and mask-plane size.
int msau_rowpair_case(int dtype, const msau_conv_pair_desc* d);
void msau_rowpair_split(const msau_conv_pair_desc* d, PairRoute* r);
int msau_rowpair_launch(hipStream_t s, const msau_conv_pair_desc* d, const PairRoute* r);
// ownerconv.hip: the first conv fed with box lists (MSAU_CONV_OWNER)
int msau_ownerconv_takes(int dtype, const msau_conv_desc* d);
int msau_ownerconv_fwd(hipStream_t s, int dtype, const msau_conv_desc* d);
// The instance families of msau_conv2d besides the tile kernel (conv_route in conv.hip picks one; DESIGN.md, "conv2d routing").
// <family>_case: the number of the instance that runs the descriptor, 0 = none; pure host arithmetic.  <family>_launch: launches
// exactly that instance -- a case it has no instance for is an MSAU_ERR_ARG error, never "try the next family".  The number packs
// what selects the instance's kernel; the family's one table of instances answers "exists" for _case and is the launch's switch.
// conv_rows.hip: row-streaming instances for the single convolutions of the 8-channel level and the two transposed convs above it
// (kchunk / rows: the packed image).  _workgroups: the grid of instance `inst` on `d`, from the task split the launch uses
int msau_rowconv_case(int dtype, const msau_conv_desc* d, int kchunk, int rows);
int msau_rowconv_launch(hipStream_t s, const msau_conv_desc* d, int kchunk, int rows, int inst);
int msau_rowconv_workgroups(const msau_conv_desc* d, int inst);
// conv_lean.hip: the chunked-K instances and the compile-time-specialised instances for the hot layer shapes
// (cch / kchunk / nchunks / CT: the generic geometry = the packed image)
int msau_conv_chunked_case(int dtype, const msau_conv_desc* d, int cch, int nchunks, int CT);
int msau_conv_chunked_launch(hipStream_t s, int dtype, const msau_conv_desc* d, int kchunk, int nchunks, int CT, int which);
int msau_conv_lean_case(int dtype, const msau_conv_desc* d, int nchunks, int CT);
int msau_conv_lean_launch(hipStream_t s, int dtype, const msau_conv_desc* d, int kchunk, int CT, int which);
// conv_first.hip: the first conv fed with the fp32 NCHW input tensor (MSAU_CONV_NCHW); one instance
int msau_firstconv_takes(int dtype, const msau_conv_desc* d);
int msau_firstconv_launch(hipStream_t s, int dtype, const msau_conv_desc* d, int real_channels);
// ---- msau_conv2d_wgrad (wgrad_route in conv_wgrad.hip picks the family and the instance; DESIGN.md, "Weight-gradient routing").
// The same contract: _case and _launch of the families besides the tile kernel, which is conv_wgrad.hip's own.
enum { WF_NONE = 0, WF_TILE = 1, WF_LEAN = 2, WF_SPECIAL = 3, WF_IN64 = 4, WF_IN64_IDS = 5, WF_ROWS = 6, WF_OWNER = 7 };   // = info[0] of msau_wgrad_route
struct WRoute {
    int family, inst;                            // WF_*, the instance's number in its family's table (lean, special, 64 -> 8, rows; else 0)
    int CTN, NKW, slices;                        // tile family: its instance and the launches of one call
    int cch, nchunks, kextc;                     // the generic geometry (wgrad_geom): all 0 = there is none
    int tiles_x, tiles_y, ntiles;                // 16 x 16 output tiles per image and of the batch = the most slabs a launch can fill
};
// wgrad_lean.hip: the compile-time-specialised instances, the dilated / stride-2 ones and the 64 -> 8 kernel; the number's low three
// bits are the family (WF_LEAN, WF_SPECIAL, WF_IN64).  _launch: ds[0..n) share one grid, n > 1 for WF_LEAN / WF_SPECIAL only
int msau_wgrad_lean_case(int dtype, const msau_wgrad_desc* d, int cch, int kextc);
int msau_wgrad_lean_launch(hipStream_t s, int dtype, const msau_wgrad_desc* const* ds, int n, const WRoute* r);
// conv_rows.hip: the row-streaming 8 -> 8 instances <RELU, KS>
int msau_rowwgrad_case(int dtype, const msau_wgrad_desc* d, int cch, int nchunks, int kextc);
int msau_rowwgrad_launch(hipStream_t s, const msau_wgrad_desc* d, int inst);
// ownerconv.hip: the first conv fed with box lists (MSAU_CONV_OWNER); one instance.  _case reads no pointer: the context behind
// d->x1 is the launch's to check
int msau_ownerconv_wgrad_case(int dtype, const msau_wgrad_desc* d, int cch, int nchunks, int kextc);
int msau_ownerconv_wgrad_launch(hipStream_t s, int dtype, const msau_wgrad_desc* d, const WRoute* r);

#define MSAU_CHECK_ARG(cond, ...)                                   \
    do {                                                            \
        if (!(cond)) return msau_set_error(MSAU_ERR_ARG, __VA_ARGS__); \
    } while (0)

#define MSAU_CHECK_LAUNCH(name)                                                         \
    do {                                                                                \
        hipError_t e__ = hipGetLastError();                                             \
        if (e__ != hipSuccess)                                                          \
            return msau_set_error(MSAU_ERR_HIP, "%s: %s", name, hipGetErrorString(e__)); \
    } while (0)

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int roundup(int a, int b) { return cdiv(a, b) * b; }

// ---- the grid-stride kernels of elementwise.hip and loss.hip: workgroup size, capped grid, storage-type dispatch ----
constexpr int kThreads = 256;

static inline int grid_for(int64_t work, int cap = 256 * 16) {
    int64_t b = cdiv64(work, kThreads);
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

#define DISPATCH_T(dtype, CALL_F32, CALL_BF16)                          \
    do {                                                                \
        if ((dtype) == MSAU_F32) { CALL_F32; }                          \
        else if ((dtype) == MSAU_BF16) { CALL_BF16; }                   \
        else return msau_set_error(MSAU_ERR_ARG, "bad dtype %d", (int)(dtype)); \
    } while (0)

// ---- LDS strides of the MFMA-operand images (conv_lean / conv_pair / conv_chunked) ---------------------------------
// A fragment read is one ds_read_b128 per lane, lane = (lr = lane & 15: pixel / weight row, lg = lane >> 4: 8-channel k-group).
// The LDS serves a ds_read_b128 in four groups of 16 lanes that are NOT lr = 0..15 of one lg: they are
// {lr 0-3, 12-15 of lg 0} + {lr 4-11 of lg 1}, the complement, and the same for lg 2 / 3 (MI355X_MICROARCH.md, LDS table); a
// group is conflict-free when its 16 lanes hit 16 different 16-byte slots of the 256-byte bank row.  lg 0 / 1 read neighbouring
// slots (k-groups cg, cg + 1 of one tap), so the stride between lr's has to put 8 consecutive lr's on the 8 EVEN slots:
// stride / 16 = 2 (mod 4).  Rounds 1-3 padded to an ODD number of slots (conflict-free if lr = 0..15 were a group): every
// fragment read was a 2-way conflict, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 0.39-0.50 on every instance
// (profiles/r04_pmc_step.txt).  Not reachable by padding: 8-channel pixels (lg 0 / 1 are different taps, i.e. pixels), lanes
// two pixels apart (STRIDE 2: the odd padding is the right one there), fp32 (two reads per fragment).
constexpr int lds_pixel_stride(int raw_bytes, int esz, int c8_per_chunk, int read_stride) {
    if (esz == 2 && c8_per_chunk >= 2 && read_stride == 1) {
        int p = raw_bytes / 16;
        while (p % 4 != 2) ++p;
        return p * 16;
    }
    return ((raw_bytes / 16) % 2 == 0) ? raw_bytes + 16 : raw_bytes;
}
// weight rows [16 x CT][k-steps x 32]: the same read with lr = output channel
constexpr int lds_wrow_stride(int nks, int esz) { return nks * 32 * esz + (esz == 2 ? 32 : 16); }

// ---- storage-type traits --------------------------------------------------------------------
template <typename T> struct Vec8;
template <> struct Vec8<float>  { typedef f32x8 type; };
template <> struct Vec8<bf16_t> { typedef bf16x8 type; };
template <typename T> struct Vec4;
template <> struct Vec4<float>  { typedef f32x4 type; };
template <> struct Vec4<bf16_t> { typedef bf16x4 type; };

// ragged batch: is position j of a W-wide grid inside a sample's extent (eh, ew)?
__device__ __forceinline__ bool pos_in_extent(int j, int W, int eh, int ew) { const int y = j / W; return y < eh && j - y * W < ew; }

template <typename T> __device__ __forceinline__ float to_f32(T v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f32(float v) { return (T)v; }

template <typename T> __device__ __forceinline__ typename Vec8<T>::type zero8() {
    typename Vec8<T>::type z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = (T)0.0f;
    return z;
}
template <typename T> __device__ __forceinline__ typename Vec8<T>::type relu8(typename Vec8<T>::type v) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = ((float)v[i] > 0.0f) ? v[i] : (T)0.0f;
    return v;
}
// bf16 ReLU on the raw bits: a negative bf16 is a negative int16, and positive bf16 values order like
// positive int16, so max(int16, 0) is exactly ReLU (-0.0 -> +0.0): one v_pk_max_i16 per two elements.
typedef short s16x8 __attribute__((ext_vector_type(8)));
template <> __device__ __forceinline__ bf16x8 relu8<bf16_t>(bf16x8 v) {
    s16x8 i = __builtin_bit_cast(s16x8, v);
    s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    i = __builtin_elementwise_max(i, z);
    return __builtin_bit_cast(bf16x8, i);
}
template <typename T> __device__ __forceinline__ typename Vec8<T>::type load8(const T* p) {
    return *reinterpret_cast<const typename Vec8<T>::type*>(p);
}
template <typename T> __device__ __forceinline__ void store8(T* p, typename Vec8<T>::type v) {
    *reinterpret_cast<typename Vec8<T>::type*>(p) = v;
}
template <typename T> __device__ __forceinline__ typename Vec4<T>::type load4(const T* p) {
    return *reinterpret_cast<const typename Vec4<T>::type*>(p);
}
template <typename T> __device__ __forceinline__ void store4(T* p, typename Vec4<T>::type v) {
    *reinterpret_cast<typename Vec4<T>::type*>(p) = v;
}

// one "k-group" step of the implicit GEMM: 8 k-values per lane.
//   bf16: a single v_mfma_f32_16x16x32_bf16 (lane l holds k = 8*(l>>4) + j)
//   f32 : eight v_mfma_f32_16x16x4_f32; instruction j takes element j of each lane's group, so the
//         4 k-slots of instruction j are k = 8*(l>>4) + j for the 4 lane groups -- A and B agree,
//         which is all the MFMA needs.  Exact fp32 products and sums.
// Inference head (MSAU_CONV_HEAD / msau_softmax_argmax_nhwc): v[0..C) logits -> probabilities in place, returns the
// index of the first maximum probability (np.argmax of the softmax output, kv_model.py:168).  Same operation order
// as softmax_nchw_kernel so that the head and MSAUWrapper.forward's `pred` agree bit for bit.
__device__ __forceinline__ int msau_head_softmax(float (&v)[16], int C) {
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 16; ++c) if (c < C) mx = fmaxf(mx, v[c]);
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) if (c < C) se += __expf(v[c] - mx);
    const float inv = 1.f / se;
    int best = 0;
    float bp = -1.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) if (c < C) {
        v[c] = __expf(v[c] - mx) * inv;
        if (v[c] > bp) { bp = v[c]; best = c; }
    }
    return best;
}

__device__ __forceinline__ f32x4 mma8(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma8(f32x8 a, f32x8 b, f32x4 c) {
#pragma unroll
    for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
    return c;
}
