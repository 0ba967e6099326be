/*
 * msau_hip.h -- C ABI of libmsau_hip.so: the MI355X (gfx950) kernels behind the MSAU train path.
 *
 * The reference (datvo06/MSAU) has no FFI layer: its hot path reaches the backend through
 * torch.nn modules.  Each entry point below replaces the backend op(s) one reference call site
 * reaches; the call site is cited as <file>:<line> relative to the reference root.  The Python
 * host side (msau_amd/) binds these with ctypes and passes raw device pointers; INTEGRATION.md
 * shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless the name ends in _host.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises.
 *  - activations are NHWC ("pixel-major, channel-minor"): [B][H][W][Cs] with Cs = stored channels,
 *    a multiple of 8 (real channels first, zero padding after).  dtype selects the STORAGE type of
 *    activations and packed weights (MSAU_F32 or MSAU_BF16); accumulation is always fp32.
 *  - every function returns 0 on success, a negative msau_status otherwise; msau_last_error()
 *    returns a thread-local message.  Nothing throws across the ABI.
 *  - functions are re-entrant per stream; handles/buffers are not thread-safe.
 */
#ifndef MSAU_HIP_H
#define MSAU_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MSAU_F32 = 0, MSAU_BF16 = 1 } msau_dtype;

typedef enum {
    MSAU_OK = 0,
    MSAU_ERR_ARG = -1,      /* bad shape / flag / alignment               */
    MSAU_ERR_LDS = -2,      /* tile does not fit the 160 KiB LDS          */
    MSAU_ERR_HIP = -3       /* a HIP runtime call failed                  */
} msau_status;

const char* msau_last_error(void);
int msau_version(void);
/* 16 hex digits: sha256 over the kernel sources + this header the library was built from (msau_amd/build.py::source_hash);
 * a binding that ships beside the sources compares the two at load time (msau_amd/_lib.py::load). */
const char* msau_source_hash(void);
/* sizeof() of the structs below as the library was compiled, for bindings that mirror them (a mirror that is too short
 * makes the library read past it): which = 0 msau_conv_desc, 1 msau_wgrad_desc, 2 msau_pack_entry, 3 msau_unpack_entry,
 * 4 msau_op, 5 msau_lrn_args, 6 msau_pool_args, 7 msau_attn_args, 8 msau_csum_args, 9 msau_reduce_args,
 * 10 msau_conv_pack_geom, 11 msau_wgrad_geom, 12 msau_conv_pair_desc, 13 msau_box_args, 14 msau_allreduce_args, 15 msau_owner_ctx,
 * 16 msau_attn_proj_bwd_args, 17 msau_dgrad2_args;
 * -1 for anything else. */
int msau_sizeof(int which);
/* LDS strides (bytes) the tile kernels give a pixel of `raw_bytes` channels / a weight row of `nks` 32-deep k-steps (csrc/msau_common.h:
 * lds_pixel_stride, lds_wrow_stride) -- exported so that a CPU test can check them against the bank model of MI355X_MICROARCH.md. */
int msau_lds_pixel_stride(int raw_bytes, int esz, int c8_per_chunk, int read_stride);
int msau_lds_wrow_stride(int nks, int esz);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution, used for: SAME conv 3x3 / dilated 3x3 / 1x1 / 4x4 forward
 * (model/layers/layers.py:82-102,152-164 -> torch.nn.Conv2d + utils.pad_2d), its data gradient,
 * the transposed-conv forward (layers.py:249-250 -> ConvTranspose2d, `ups`=2) and the
 * transposed-conv data gradient (`stride`=2).  The concat of model/model.py:147,242,251 is folded
 * in as a second source pointer.
 *
 *   v   = sum_{tap,c} in(b, oy*stride + ky*dil - pad_t, ox*stride + kx*dil - pad_l, c) * W[co][tap][c]
 *         (+ bias[co])
 *   in  = concat(x1, x2) along channels, optionally ReLU'd on load (MSAU_CONV_RELU_IN); with ups=2 the
 *         input is the zero-stuffed image (value at even virtual coords only)
 *   v  *= (mask_a > 0)            if MSAU_CONV_MASK_A        (backward through a ReLU on the conv input)
 *   v  += add                     if MSAU_CONV_ADD           (forward: residual; backward: other grad path)
 *   v  += y_old                   if MSAU_CONV_ACCUM
 *   v   = max(v, 0)               if MSAU_CONV_RELU_OUT
 *   v  *= (mask_b > 0)            if MSAU_CONV_MASK_B        (backward through the ReLU that produced y's tensor)
 *   y   = v                       (mask_a, add, mask_b, y share y's shape [B][Hout][Wout][Cout])
 * ------------------------------------------------------------------------------------------ */
enum {
    MSAU_CONV_RELU_IN  = 1,
    MSAU_CONV_RELU_OUT = 2,
    MSAU_CONV_ADD      = 4,
    MSAU_CONV_ACCUM    = 8,
    MSAU_CONV_MASK_A   = 16,
    MSAU_CONV_MASK_B   = 32,
    MSAU_CONV_DOUT     = 128,   /* two output tensors (the data gradient of a conv over concat(x1, x2), one launch instead
                                   of two): the Cout stored rows are the channels of y (first half) and y2 (second half),
                                   each [B][Hout][Wout][Cout/2]; `flags` / add / mask_b apply to y, `flags2` (ACCUM and
                                   MASK_B only) / mask_b2 to y2.  Single-source 1x1 / 3x3 convs with C1 == Cout/2 in
                                   {8, 16, 32}; msau_conv2d_launch_info: info[7] & 2 when the launch can take it. */
    MSAU_CONV_LRN      = 256,   /* second output y2 = LocalResponseNorm(size = Cout)(y) (layers.py:145,161-162: the LRN
                                   behind the level-entry conv), computed from the storage-rounded y with lrn_alpha_over_n,
                                   lrn_beta, lrn_k: y2 = y * (k + alpha/n * sum over [c - n/2, c + (n-1)/2] of y^2)^-beta.
                                   Only with RELU_IN as the other flag; msau_conv2d_launch_info: info[7] & 4 when the
                                   launch can take it (otherwise run msau_lrn_fwd on y). */
    MSAU_CONV_POOL     = 512,   /* further output pool_y = MaxPool2d(2,2) of the zero-padded y (model/model.py:158-160),
                                   [B][ceil(Hout/2)][ceil(Wout/2)][Cout], and, when pool_idx is not NULL, the position
                                   0..3 (= 2*dy + dx) of the first maximum per element (what msau_maxpool2x2_bwd reads);
                                   info[7] & 8 when the launch can take it (otherwise run msau_maxpool2x2_fwd on y). */
    MSAU_CONV_IDS      = 1024,  /* x1 is an int32 id mask [B][Hin][Win] instead of a tensor: input channel c of a pixel is
                                   (id == c), ids outside [0, C1) are empty pixels -- the one-hot chargrid is synthesised in
                                   LDS, never painted nor read, and the result equals the dense launch bit for bit.  C1 = 64,
                                   3x3, <= 16 output channels; info[7] & 16.  msau_conv2d_wgrad takes the same flag. */
    MSAU_CONV_OWNER    = 2048,  /* the net's first conv fed with BOX LISTS instead of a painted tensor (csrc/ownerconv.hip): x1 is a
                                   HOST pointer to an msau_owner_ctx -- per pixel the index of the owning box (msau_raster_owner), the
                                   box list, the feature table.  The piecewise-constant embedding chargrid (data_generator_funsd_bert.py:
                                   64-93,240; 1536 bytes per pixel at 768 channels) is never painted: the forward gathers per-tap partial
                                   products from a [feature row][tap][co] table, the weight gradient sums the output gradient per box
                                   and tap.  3x3, stride 1, C1 -> 8; other flags: RELU_OUT, and EXTENT (ragged batch: a pixel outside its sample's
                                   extent is stored as 0 and gathers nothing, taps stop at the document's edge; the owner map must come
                                   from msau_raster_owner_ext, and the weight gradient relies on g being 0 outside the extents); also on
                                   msau_wgrad_desc.flags (x1 = the same context; EXTENT needs no pointer there; the first
                                   msau_owner_slabs(d) slabs are written -- the slab reduction must be told).
                                   msau_conv2d_launch_info: info[7] & 32 when the launch can take it. */
    MSAU_CONV_NCHW     = 4096,  /* the net's first conv fed with the API's input tensor itself (csrc/conv_first.hip): x1 is fp32 NCHW
                                   [B][C][Hin][Win] with C = head_classes real channels (<= C1 = 64 stored; the missing ones are zero), and
                                   y2, if not NULL, receives its NHWC copy in the storage dtype -- what msau_nchw_to_nhwc would have
                                   written, for the weight gradient of the backward.  bf16, 3x3 SAME stride 1, 64 -> 8, Win % 4 == 0,
                                   16 <= Win <= 320 as far as the three-row LDS ring fits (msau_firstconv_takes decides;
                                   msau_conv2d_launch_info reports it); other flags: RELU_OUT only; results equal msau_nchw_to_nhwc + the dense launch bit for bit.
                                   msau_conv2d_launch_info: info[7] & 64 when the launch can take it. */
    MSAU_CONV_WGRAD    = 8192,  /* with MSAU_CONV_DOUT on the two-output data gradient of the 1x1 coupling conv over concat(8, 8) -> 8
                                   (model/model.py:143-148,246-252): the conv's WEIGHT gradient rides on this launch.  Its g operand is
                                   this launch's input x1 and the second source of the forward conv is already here as mask_b2 (the
                                   ReLU mask of y2 is the forward tensor itself), so only the first source is read in addition: wg_x1.
                                   wg_slabs = msau_conv2d_rider_slabs() slabs of [2 chunks][8][16] fp32 in the layout msau_wgrad_reduce
                                   expects for that conv (cch 8, kext 16, ones column 8 of chunk 0); the stand-alone weight-gradient
                                   launch, its read of g and of the second source disappear.  Row-streaming 8-channel bf16 instance only. */
    MSAU_CONV_ELU      = 32768, /* activation_name="elu" (model/model.py:412-416): MSAU_CONV_RELU_OUT means v = ELU(v) (alpha 1: v > 0 ? v : exp(v) - 1)
                                   and MSAU_CONV_MASK_B (the tensor's own stored output y) means v *= (y > 0 ? 1 : y + 1), the derivative of ELU at
                                   the pre-activation.  MSAU_CONV_RELU_IN / MASK_A stay ReLU: the reference's residual block starts with a
                                   hard-wired torch.nn.ReLU (model/model.py:35,39).  Generic kernel only (no fused / row / lean instance). */
    MSAU_CONV_EXTENT   = 65536, /* ragged batch: `extent` ([B][2] int32 (h, w) of each sample on the OUTPUT grid) -- applied LAST, after bias, masks,
                                   add, accumulate and activation: a pixel (oy, ox) with oy >= h or ox >= w of its sample is stored as 0.  For
                                   forward convs, transposed convs (ups = 2) and data gradients (stride = 2 included: its output is the deconv
                                   input's grid).  Implemented by the generic tile kernel (conv.hip) and by the box-list instance (MSAU_CONV_OWNER,
                                   ownerconv.hip): every other instance refuses the flag, so it does not combine with HEAD / DOUT / LRN /
                                   POOL / IDS / NCHW / WGRAD (msau_conv2d_launch_info
                                   info[7] bit 7 says whether the instance taking the descriptor implements it). */
    MSAU_CONV_HEAD     = 64     /* inference head (kv_model.py:305-313): besides y, write softmax over the Cout real
                                   channels of the (storage-rounded) result to head_probs (fp32 [B][Hout][Wout][Cout],
                                   dense) and the index of its first maximum to head_argmax (uint8 [B][Hout][Wout]).
                                   Forward convs with Cout <= 16 and no other epilogue flag; see
                                   msau_conv2d_launch_info: info[7] != 0 when the launch can take the flag, otherwise
                                   run msau_softmax_argmax_nhwc on y. */
};

typedef struct {
    int32_t B, Hin, Win, Hout, Wout;
    int32_t C1, C2;             /* stored channels of x1 / x2 (C2 = 0: single source)               */
    int32_t Cout;               /* stored output channels                                           */
    int32_t KH, KW, dil;
    int32_t pad_t, pad_l;
    int32_t stride;             /* 1 | 2                                                            */
    int32_t ups;                /* 1 | 2                                                            */
    int32_t flags;
    const void* x1;
    const void* x2;
    const void* wpack;          /* geometry.bytes bytes, written by msau_pack_params           */
    const float* bias;          /* [Cout] fp32 or NULL                                              */
    const void* add;
    const void* mask_a;
    const void* mask_b;
    void* y;
    float* head_probs;          /* MSAU_CONV_HEAD only: fp32 [B][Hout][Wout][head_classes]          */
    uint8_t* head_argmax;       /* MSAU_CONV_HEAD only: uint8 [B][Hout][Wout]                       */
    int32_t head_classes;       /* MSAU_CONV_HEAD only: real classes (<= Cout, <= 16)               */
    int32_t flags2;             /* MSAU_CONV_DOUT only: epilogue flags of y2                        */
    void* y2;                   /* MSAU_CONV_DOUT only                                              */
    const void* mask_b2;        /* MSAU_CONV_DOUT only                                              */
    float lrn_alpha_over_n, lrn_beta, lrn_k;   /* MSAU_CONV_LRN only (y2 is the LRN output)          */
    int32_t reserved0;
    void* pool_y;               /* MSAU_CONV_POOL only                                              */
    uint8_t* pool_idx;          /* MSAU_CONV_POOL only, may be NULL                                 */
    const void* wg_x1;          /* MSAU_CONV_WGRAD only: the forward conv's first source [B][H][W][8]  */
    float* wg_slabs;            /* MSAU_CONV_WGRAD only: [msau_conv2d_rider_slabs()][2][8][16] partial sums, one slab per workgroup */
    int32_t wg_nslabs;          /* MSAU_CONV_WGRAD only: the slab count the caller allocated: the launch refuses to write another number */
    int32_t reserved1;
    const int32_t* extent;      /* MSAU_CONV_EXTENT only: [B][2] (h, w) of every sample on the output grid (ABI v11)        */
} msau_conv_desc;
/* number of slabs an MSAU_CONV_WGRAD launch of this descriptor writes (= its workgroups); 0 if no instance takes the flag */
int msau_conv2d_rider_slabs(int dtype, const msau_conv_desc* d);

/* Geometry of the packed weight image the conv kernel expects for a given layer.
 * rows = roundup16(Cout) padded up to a power-of-two number of 16-row tiles; K is laid out as
 * [chunk][tap][channel-in-chunk] with `cch` channels per chunk, padded to a multiple of 32.        */
typedef struct {
    int32_t cch;        /* channels staged per K-chunk (multiple of 8)      */
    int32_t nchunks;
    int32_t kchunk;     /* padded K elements per chunk (multiple of 32)     */
    int32_t rows;       /* padded rows                                      */
    int64_t bytes;      /* total bytes of the packed image                  */
} msau_conv_pack_geom;

int msau_conv_pack_geometry(int dtype, int C1_stored, int C2_stored, int Cout_stored, int KH, int KW, int dil,
                            int stride, int ups, msau_conv_pack_geom* out);
int msau_conv2d(void* stream, int dtype, const msau_conv_desc* d);
/* which template instance msau_conv2d launches for this descriptor (for profiling / roofline):
 * info[0] = CT (16-row output-channel tiles), info[1] = PT (pixel tiles per wave: tile = 4*PT x 16),
 * info[2] = dynamic LDS bytes, info[3] = workgroups, info[4] = channel chunk, info[5] = chunks,
 * info[6] = 1 if a compile-time-specialised "lean" instance (conv_lean.hip) takes the launch, 2 if the chunked-K instance does,
 *           3 if a row-streaming instance (conv_rows.hip) does; 0 otherwise: the generic tile kernel, and also a descriptor
 *           msau_conv2d refuses or gives to the box-list (MSAU_CONV_OWNER) or NCHW (MSAU_CONV_NCHW) instance,
 * info[7] = bit 0: that instance implements MSAU_CONV_HEAD for this descriptor, bit 1: MSAU_CONV_DOUT,
 *           bit 2: MSAU_CONV_LRN, bit 3: MSAU_CONV_POOL, bit 4: MSAU_CONV_IDS, bit 5: MSAU_CONV_OWNER, bit 6: MSAU_CONV_NCHW,
 *           bit 7: MSAU_CONV_EXTENT (the instance that takes the descriptor with the flag added implements it) */
int msau_conv2d_launch_info(int dtype, const msau_conv_desc* d, int32_t* info8);

/* ------------------------------------------------------------------------------------------
 * Two chained 3x3 SAME convolutions C -> C -> C (C stored channels in {8, 16, 32}) in one launch: the residual block
 * of model/model.py:37-50 with res_depth 2 (forward) and its two data gradients (backward).  The intermediate tensor
 * `mid` is written once and consumed from LDS, never re-read from HBM.
 *   t   = W1 * in(x) + b1            in(x) = max(x, 0) if MSAU_PAIR_RELU_IN else x ;  b1 may be NULL
 *   t   = max(t, 0)                  if MSAU_PAIR_RELU_MID      (forward: the first conv's ReLU)
 *   t  *= (mask_mid > 0)             if MSAU_PAIR_MASK_MID      (backward: through that ReLU)
 *   mid = t                          ([B][H][W][C], zero outside the image: the second conv's SAME padding)
 *   y   = epilogue(W2 * mid + b2)    flags2 = MSAU_CONV_{MASK_A, ADD, ACCUM, RELU_OUT, MASK_B, POOL} exactly as msau_conv2d
 * w1 / w2 are the packed images msau_pack_params writes for a single-source 3x3 conv C -> C (forward or flipped
 * data-gradient image).  msau_conv_pair_applicable: 1 if an instance takes the descriptor (shape, flags, the riders' operands).
 * ------------------------------------------------------------------------------------------ */
enum { MSAU_PAIR_RELU_IN = 1, MSAU_PAIR_RELU_MID = 2, MSAU_PAIR_MASK_MID = 4,
       MSAU_PAIR_LRN_BWD = 16,  /* backward flag set only: x0 (whose gradient this launch produces) is the output of
                                   LocalResponseNorm(size = C) applied to lrn_a (layers.py:145,161-162), and nothing else
                                   contributes to its gradient: the launch runs the LRN backward on the storage-rounded result in
                                   its epilogue and writes lrn_da (gradient w.r.t. lrn_a) INSTEAD of y -- the msau_lrn_bwd launch,
                                   its read of dy and the write of dy disappear.  The row-streaming backward instances have it, at 8 and
                                   (unless MSAU_LRN_BWD16=0) at 16 channels (msau_conv_pair_applicable says so); lrn_alpha_over_n / lrn_beta / lrn_k as in msau_conv_desc */
       MSAU_PAIR_WGRAD1 = 32,   /* backward flag set only: the weight gradient of the block's FIRST conv in the same launch -- its g
                                   operand is the intermediate gradient this launch produces, so that tensor is neither written
                                   (`mid` is left untouched) nor re-read; wg1_x = the block's forward input x0 (ReLU applied on load),
                                   wg1_slabs = msau_conv_pair_wgrad_slabs() slabs of [8][80] fp32 in the layout msau_wgrad_reduce expects
                                   (kext 80, ones column 72).  Row-streaming 8-channel instance only. */
       MSAU_PAIR_COUPLE = 64,   /* forward flag set only: the coupling conv that follows the block in a coupled stage
                                   (model/model.py:143-148,246-252) rides on this launch --
                                       z = max(Wc * concat(cpl_prev, y) + bc, 0)           ([B][H][W][C], written to cpl_y)
                                   computed from the storage-rounded y exactly as the stand-alone 1x1 launch reads it; y itself is still
                                   written (the backward reads it).  cpl_w / cpl_b = the packed image / bias msau_pack_params writes
                                   for a 1x1 conv over concat(C, C) -> C.  With cpl_pool_y != NULL also the zero-padded MaxPool2d(2,2)
                                   of z (cpl_pool_idx: the 1-byte positions, may be NULL), as MSAU_CONV_POOL does for y.  The row-streaming
                                   8- and 16-channel instances and the 32-channel bf16 tile pair have it (msau_conv_pair_applicable
                                   says so); not together with MSAU_CONV_POOL in flags2. */
       MSAU_PAIR_DCOUPLE = 128, /* backward flag set only: the block's output y feeds nothing but a coupling conv z = ReLU(Wc concat(prev, y) + bc)
                                   whose two-output data gradient (MSAU_CONV_DOUT) becomes the PROLOGUE of this launch: the input tile is read
                                   from dcp_dz = d(z) (masked by z > 0 already) instead of x, and
                                       g = d(y) = (Wc[:, y]^T d(z)) . [dcp_mask > 0]   (dcp_mask = y)   feeds the two data gradients below AND is
                                                                                      written to x -- the weight gradient of the block's second
                                                                                      conv reads it there AFTER this launch
                                       d(prev)  =  Wc[:, prev]^T d(z)                 written to dcp_dprev (plain write: nothing accumulated, no mask)
                                   dcp_w = the packed two-output data-gradient image of the coupling conv (msau_conv_pack_geometry(C, 0, 2C, 1x1)).
                                   The 32-channel bf16 tile pair has it (msau_conv_pair_applicable says so). */
       MSAU_PAIR_TILES = 8 };   /* take the tile kernels (conv_pair.hip) even where the row-streaming kernel has an instance: the
                                   forward and the backward launch of one block must agree on the layout of the mask planes, so a
                                   caller whose forward carries a flag only the tile kernels implement (MSAU_CONV_POOL) sets this on
                                   both descriptors */
typedef struct {
    int32_t B, H, W, C;
    int32_t flags1, flags2;
    const void* x;
    const void* w1;
    const float* b1;
    const void* mask_mid;
    void* mid;
    const void* w2;
    const float* b2;
    const void* add;
    const void* mask_a;
    const void* mask_b;
    void* y;
    void* pool_y;               /* flags2 & MSAU_CONV_POOL (forward flag set only): MaxPool2d(2,2) of the zero-padded y, */
    uint8_t* pool_idx;          /* [B][ceil(H/2)][ceil(W/2)][C] and the 1-byte positions (may be NULL), as msau_conv2d   */
    uint8_t* bits_mid;          /* both NULL, or ReLU masks as bit planes [B][H][W][C/8] (bit c%8 of byte c/8 = element > 0): */
    uint8_t* bits_a;            /* the forward flag set WRITES (mid > 0) and (x > 0); the backward flag set READS them     */
                                /* instead of the tensors mask_mid / mask_a (which may then be NULL)                       */
    const void* lrn_a;          /* MSAU_PAIR_LRN_BWD: the LRN's input [B][H][W][C] ...                                     */
    void* lrn_da;               /* ... and the gradient w.r.t. it (written; y is not)                                      */
    float lrn_alpha_over_n, lrn_beta, lrn_k;
    int32_t reserved0;
    const void* wg1_x;          /* MSAU_PAIR_WGRAD1: x0, [B][H][W][C]                                                     */
    float* wg1_slabs;           /* [msau_conv_pair_wgrad_slabs()][C][80] partial sums, one slab per workgroup             */
    int32_t wg1_nslabs;         /* the slab count the caller allocated: the launch refuses to write another number        */
    int32_t reserved1;
    const void* cpl_prev;       /* MSAU_PAIR_COUPLE: the coupling conv's first source (the previous stage's tensor)      */
    const void* cpl_w;          /* ... its packed weight image (1x1, concat(C, C) -> C) and bias                          */
    const float* cpl_b;
    void* cpl_y;                /* ... its output z                                                                       */
    void* cpl_pool_y;           /* ... NULL, or the pooled z [B][ceil(H/2)][ceil(W/2)][C]                                 */
    uint8_t* cpl_pool_idx;      /* ... and its 1-byte positions (may be NULL)                                             */
    const void* dcp_dz;         /* MSAU_PAIR_DCOUPLE: gradient of the coupling conv's output, [B][H][W][C]                */
    const void* dcp_w;          /* ... its packed two-output data-gradient image (2C rows)                                */
    const void* dcp_mask;       /* ... the block's forward output y (ReLU mask of d(y))                                   */
    void* dcp_dprev;            /* ... gradient w.r.t. the coupling conv's first source (written)                         */
} msau_conv_pair_desc;
int msau_conv_pair_applicable(int dtype, const msau_conv_pair_desc* d);
int msau_conv_pair(void* stream, int dtype, const msau_conv_pair_desc* d);
/* bytes of ONE mask plane (bits_mid or bits_a) for this descriptor's shape.  The planes are private between the forward and
 * the backward launch of one residual block and their layout follows the instance that takes the descriptor once it has planes
 * (it need not have them yet): a byte per (pixel, 8-channel group) for the tile kernels (conv_pair.hip) and for a shape no
 * instance takes, 32 bytes of lane ballots per (row, strip) for the row-streaming bf16 kernels (conv_rows.hip; strips of 30
 * columns at 8 channels, of 14 at 16).  Allocate with this, never from the layout comment above. */
int64_t msau_conv_pair_bits_bytes(int dtype, const msau_conv_pair_desc* d);
/* number of slabs an MSAU_PAIR_WGRAD1 launch of this descriptor writes (= its workgroups); 0 if no instance takes the flag */
int msau_conv_pair_wgrad_slabs(int dtype, const msau_conv_pair_desc* d);
/* which instance takes the descriptor: 0 none, 1 a tile kernel (conv_pair.hip), 2 a row-streaming kernel (conv_rows.hip) */
int msau_conv_pair_instance(int dtype, const msau_conv_pair_desc* d);
/* The library reads its MSAU_* environment switches once.  msau_reload_env() makes the switches of the row-streaming kernels
 * (conv_rows.hip: MSAU_PAIR_ROWS, MSAU_CONV_ROWS, MSAU_WGRAD_ROWS, MSAU_WGRAD_ROWS4, MSAU_DOUT_ROWS, MSAU_DECONV_ROWS, MSAU_ROWS_SH,
 * MSAU_ROWS_SH16, MSAU_ROWS_WAVES, MSAU_ROWS_MIN_TASKS, MSAU_ROWS_MAXC, MSAU_PAIR_WGRAD, MSAU_PAIR_COUPLE, MSAU_COUPLE_WGRAD,
 * MSAU_LRN_BWD16) be read again on the next call: for tests and A/B tools that change them inside one process.  Every other
 * switch of the library, those of conv_pair.hip among them, is read once per process. */
void msau_reload_env(void);

/* ------------------------------------------------------------------------------------------
 * Weight / bias gradient of the same convolution (autograd of torch.nn.Conv2d reached from
 * train_chargrid_funsd_msau.py:57 `loss.backward()`), and with stride=2 of the transposed conv
 * (roles of input and output-gradient swapped, see msau_amd/plan.py).
 *   slab[s][chunk][co][k]  partial sums over the pixel tiles workgroup s visited (deterministic, no atomics)
 *   The input channels are cut into nchunks chunks of cch (msau_wgrad_geometry; a chunk never straddles x1 | x2), and every
 *   chunk has its own [Cout][kext] block: k = tap * cch + channel-in-chunk for k < taps * cch, column taps * cch holds
 *   sum(g) = dbias (the "ones" column, the same value in every chunk), the columns up to kext = taps * cch + 8 rounded up to
 *   16 are padding (zero, or never written).  One slab is nchunks * Cout * kext floats.
 * msau_wgrad_reduce() sums the slabs and scatters into the flat fp32 gradient buffer.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t B, Hin, Win, Hout, Wout;
    int32_t C1, C2, Cout;
    int32_t KH, KW, dil, pad_t, pad_l, stride;
    int32_t flags;              /* MSAU_CONV_RELU_IN; MSAU_CONV_IDS (x1 = int32 id mask, C1 = 64, Cout = 8, 3x3);
                                   MSAU_CONV_OWNER (x1 = host msau_owner_ctx), with it MSAU_CONV_EXTENT (no pointer: the
                                   per-box sums run in an order anchored on the canvas, independent of what a box covers
                                   outside its document) */
    const void* x1;
    const void* x2;
    const void* g;              /* [B][Hout][Wout][Cout] gradient w.r.t. the conv's pre-activation  */
    float* slabs;               /* [nslabs][nchunks][Cout][kext] fp32                               */
    int32_t nslabs;             /* number of workgroups per chunk to launch (<= tiles)              */
} msau_wgrad_desc;

typedef struct {
    int32_t cch, nchunks;
    int32_t kext;               /* columns per row of ONE chunk: taps*cch + 8, rounded to 16        */
    int32_t max_slabs;          /* number of pixel tiles (upper bound for nslabs)                   */
    int64_t slab_bytes;         /* bytes of ONE slab                                                */
    int32_t lean;               /* 1: a compile-time-specialised instance (wgrad_lean.hip) takes it; 2: the row-streaming
                                   instance (conv_rows.hip; needs d->nslabs set) */
    int32_t reserved;
} msau_wgrad_geom;

int msau_wgrad_geometry(int dtype, const msau_wgrad_desc* d, msau_wgrad_geom* out);
int msau_conv2d_wgrad(void* stream, int dtype, const msau_wgrad_desc* d);
/* Which kernel msau_conv2d_wgrad launches for the descriptor (host only: no launch, no device, the pointers are not read;
 * d->nslabs >= 1 as for the launch).  msau_conv2d_wgrad, msau_wgrad_geometry (its `lean`) and msau_conv2d_wgrad_groupable
 * take their decision from it.  Returns 0, or the error the launch would return (info[0] = 0).
 *   info[0] family: 0 refused, 1 the generic tile kernel, 2 a lean instance, 3 a dilated / stride-2 lean instance, 4 the
 *           64 -> 8 role-swapped instance, 5 the same fed with ids (MSAU_CONV_IDS), 6 the row-streaming instance, 7 the
 *           box-list weight gradient (MSAU_CONV_OWNER)
 *   info[1], info[2]  generic kernel: CTN (16-channel row tiles per slice as instantiated: 3 -> 4, 5..8 -> 8) and NKW (rounds of
 *           4 k-tiles per wave: 1, 2, 3, 5, 10); else 0
 *   info[3] 1: the generic kernel's compact form (dil >= 16: one 16 x 16 input block per tap)
 *   info[4] launches = output-channel slices (generic kernel: 128 channels each in bf16, 64 in fp32, 32 in fp32 compact; else 1)
 *   info[5], info[6], info[7]  cch, nchunks, kext of the msau_wgrad_geom struct; set whenever the geometry exists */
int msau_wgrad_route(int dtype, const msau_wgrad_desc* d, int32_t info[8]);
/* Up to 4 weight gradients of one shape (everything but the tensors equal: msau_conv2d_wgrad_groupable(a, b) != 0) in ONE
 * grid -- the level-2/3 launches have 64-107 workgroups each and otherwise queue behind each other.  Same slabs, same bits
 * as n separate launches. */
int msau_conv2d_wgrad_groupable(int dtype, const msau_wgrad_desc* a, const msau_wgrad_desc* b);
int msau_conv2d_wgrad_group(void* stream, int dtype, const msau_wgrad_desc* const* ds, int n);

/* ------------------------------------------------------------------------------------------
 * Parameter packing (fp32 master parameters in the reference's OIHW / IOHW layouts -> packed
 * images for msau_conv2d) and gradient un-packing (slabs -> flat fp32 gradient in the reference's
 * layouts).  One launch handles a whole table.  The table lives in DEVICE memory.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int64_t src_off;        /* element offset of the parameter in the flat fp32 parameter buffer         */
    int64_t dst_off;        /* BYTE offset of the packed image in the pack arena                        */
    int32_t kind;           /* 0 = weight image, 1 = bias vector (fp32, padded to rows_store)           */
    int32_t dim0, dim1;     /* parameter dims 0 and 1 (OIHW: O,I ; ConvTranspose IOHW: I,O)             */
    int32_t KH, KW;
    int32_t row_is_dim0;    /* 1: image rows index dim0 (conv fwd, deconv dgrad); 0: rows index dim1   */
    int32_t flip;           /* 1: taps reversed (data-gradient / transposed-conv forward)              */
    int32_t row_off;        /* first parameter index (along the row dim) covered by this image          */
    int32_t rows_real;      /* valid rows                                                               */
    int32_t rows_pad;       /* geometry.rows                                                            */
    int32_t k1_real, k1_store, k2_real, k2_store;   /* channel split of the K dim (source 1 | source 2)  */
    int32_t cch, nchunks, kchunk;
    int32_t dtype;
} msau_pack_entry;

int msau_pack_params(void* stream, const float* flat_params, void* pack_arena,
                     const msau_pack_entry* table_dev, int n_entries, int max_elems_per_entry);

typedef struct {
    int64_t slab_off;       /* element offset of slab 0 in the fp32 slab arena                          */
    int64_t w_off;          /* element offset of the weight gradient in the flat gradient buffer        */
    int64_t b_off;          /* element offset of the bias gradient, or -1                               */
    int64_t b_src_off;      /* bias partial sums: element (slab s, channel r) of the slab arena is      */
    int64_t b_slab_stride;  /*   b_src_off + s*b_slab_stride + r*b_elem_stride, s < b_nslabs            */
    int32_t b_elem_stride;  /*   (the "ones" column of a wgrad slab, or msau_channel_sum partials)      */
    int32_t b_nslabs;
    int32_t b_count;        /* number of bias elements (conv: rows_real; transposed conv: its out channels) */
    int32_t nslabs;
    int32_t slab_elems;     /* nchunks * Cout_store * kext                                              */
    int32_t kext;
    int32_t dim0, dim1, KH, KW;
    int32_t row_is_dim0;    /* 1: slab rows index dim0, slab channels index dim1 ; 0: the other way     */
    int32_t rows_real;
    int32_t k1_real, k1_store, k2_real, k2_store;
    int32_t cch, nchunks;
    int32_t accumulate;     /* 1: add to the existing gradient (second wgrad of the same parameter)     */
} msau_unpack_entry;

int msau_wgrad_reduce(void* stream, const float* slab_arena, float* flat_grads,
                      const msau_unpack_entry* table_dev, int n_entries, int max_elems_per_entry);

/* partial per-channel sums of a gradient tensor (bias gradient of the transposed conv, whose wgrad
 * runs with swapped roles): partials[blk][c] = sum over the pixels block blk visited; nblk rows. */
int msau_channel_sum(void* stream, int dtype, const void* g, int64_t npix, int Cs, float* partials, int nblk);

/* ------------------------------------------------------------------------------------------
 * Layout conversion at the boundary: the reference API speaks NCHW fp32
 * (train_chargrid_funsd_msau.py:50-53, model/model.py:435-437).
 * ------------------------------------------------------------------------------------------ */
int msau_nchw_to_nhwc(void* stream, int dtype, const float* src, void* dst, int B, int C, int Cs, int H, int W);
int msau_nhwc_to_nchw(void* stream, int dtype, const void* src, float* dst, int B, int C, int Cs, int H, int W);
/* gradient of nhwc_to_nchw: dst[b][h][w][c] (+)= src[b][c][h][w] ; padded channels written as 0 */
int msau_nchw_grad_to_nhwc(void* stream, int dtype, const float* src, void* dst, int B, int C, int Cs, int H, int W,
                           int accumulate);

/* ------------------------------------------------------------------------------------------
 * LocalResponseNorm(size = n) across channels, alpha=1e-4, beta=0.75, k=1
 * (model/layers/layers.py:145,161-162 -> torch.nn.LocalResponseNorm).  C = real channels.
 *   y_c = a_c * (k + alpha/n * sum_{c' in [c-n/2, c+(n-1)/2]} a_c'^2)^-beta
 * ------------------------------------------------------------------------------------------ */
int msau_lrn_fwd(void* stream, int dtype, const void* a, void* y, int64_t npix, int C, int Cs, int n,
                 float alpha, float beta, float k);
int msau_lrn_bwd(void* stream, int dtype, const void* a, const void* dy, void* da, int64_t npix, int C, int Cs,
                 int n, float alpha, float beta, float k);

/* ------------------------------------------------------------------------------------------
 * 2x2 stride-2 max pool after zero SAME padding (model/model.py:158-160).  idx = argmax position
 * (0..3, first maximum in row-major window order, as torch CPU) kept as one byte per output element.
 * bwd: dx = ((accumulate & 1) ? dx : 0) + scatter(dy); dx *= (mask > 0) if mask != NULL -- or, with bit 1 of `accumulate` set (the
 * masked tensor is the output of an ELU, activation_name="elu"), dx *= (mask > 0 ? 1 : mask + 1).
 * ------------------------------------------------------------------------------------------ */
int msau_maxpool2x2_fwd(void* stream, int dtype, const void* x, void* y, uint8_t* idx, int B, int H, int W, int Cs);
int msau_maxpool2x2_bwd(void* stream, int dtype, const void* dy, const uint8_t* idx, void* dx, const void* mask,
                        int B, int H, int W, int Cs, int accumulate);
/* as msau_maxpool2x2_bwd, for a ragged batch: extent [B][2] (h, w) of every sample on the pool's INPUT grid; dx is written as 0
 * at the pixels outside it (the gradient a window sends to its zero padding, which an ELU's MASK_B would not remove) */
int msau_maxpool2x2_bwd_ext(void* stream, int dtype, const void* dy, const uint8_t* idx, void* dx, const void* mask,
                            int B, int H, int W, int Cs, int accumulate, const int32_t* extent);

/* ------------------------------------------------------------------------------------------
 * Bottleneck self-attention core (model/layers/attention.py:156-162), given the 1x1 projections
 * f, g ([B][N][Ds]) and h ([B][N][Cs]):   y = x + h . softmax_rows(g^T f)
 * Two passes, no N x N matrix: stats (row max m_i and row sum Z_i of exp), then the output.
 * bwd: df, dg, dh from dy (the residual path dx += dy is the caller's).  ws: B*N*(Cs+4) floats.
 * ------------------------------------------------------------------------------------------ */
int msau_selfattn_fwd(void* stream, int dtype, const void* f, const void* g, const void* h, const void* x, void* y,
                      float* stats /* [B][N][2] */, int B, int N, int Ds, int Cs);
int msau_selfattn_bwd(void* stream, int dtype, const void* f, const void* g, const void* h, const void* dy,
                      const float* stats, void* df, void* dg, void* dh, float* ws, int B, int N, int Ds, int Cs);
/* Ragged batch: the bottleneck grid is [H][W] = N positions per sample and sample b covers (h_b, w_b) = extent[b] of it.  Keys
 * j = (j / W, j % W) outside the sample's extent are excluded from the softmax (P[i][j] = 0: statistics and all four sweeps),
 * y = x at those columns and dh = 0 at rows outside the extent.  f, g, h, x, dy must be 0 outside the extents (the plan's
 * invariant); then every output is 0 there.  Masked instances of the same kernels; extent = NULL is msau_selfattn_fwd / _bwd. */
int msau_selfattn_fwd_ext(void* stream, int dtype, const void* f, const void* g, const void* h, const void* x, void* y,
                          float* stats, int B, int N, int Ds, int Cs, const int32_t* extent, int W);
int msau_selfattn_bwd_ext(void* stream, int dtype, const void* f, const void* g, const void* h, const void* dy,
                          const float* stats, void* df, void* dg, void* dh, float* ws, int B, int N, int Ds, int Cs,
                          const int32_t* extent, int W);

/* Which kernel family msau_selfattn_fwd / _bwd (and _ext) run for (dtype, N, Ds, Cs): 0 = a compile-time VALU instance, 1 = the
 * run-time "any width" kernels, 2 = the bf16 MFMA sweeps; -1 for an unknown dtype.  The dispatchers themselves call it. */
int msau_selfattn_route(int dtype, int N, int Ds, int Cs);

/* Ragged batch: dst[b][p][y][x][:] = (y < h_b && x < w_b) ? src[b][p][y][x][:] : 0 for a tensor of `planes` planes of H x W pixels of
 * `pixel_bytes` bytes each per sample (NHWC activation: planes 1, pixel_bytes Cs * esz; int64 labels: 1, 8; NCHW fp32: C, 4).
 * extent [B][2] int32 (h, w).  src == dst is allowed (in place).  pixel_bytes must be a multiple of 4. */
int msau_extent_copy(void* stream, const void* src, void* dst, int B, int planes, int H, int W, int pixel_bytes, const int32_t* extent);

/* The data gradients of the attention block's three 1x1 projections (model/layers/attention.py:152-154: f, g: C -> C/8, h: C -> C, all
 * reading the same tensor x) as ONE launch instead of three accumulating msau_conv2d launches:
 *   v  = Wf^T df + Wg^T dg + Wh^T dh        (fp32 accumulation over K = C/8 + C/8 + C in one MFMA chain)
 *   v += add                  if add        (the attention residual y = o + x: dy)
 *   v += dx_old               if accumulate (an earlier contribution to dx, e.g. the decoder's transposed conv)
 *   v  = mask_b > 0 ? v : 0   if mask_b     (ReLU of x's producer)
 *   dx = round(v)
 * wf_pack / wg_pack / wh_pack: the packed DATA-GRADIENT images of the three convs exactly as msau_conv2d takes them
 * (msau_conv_pack_geometry(dtype, C/8 or C, 0, C, 1, 1, 1, 1, 1): one chunk, 64 rows, kchunk 32 / 32 / 64) -- the launch reads its
 * weight fragments straight from them.  bf16, C = 64 only (MSAU_ERR_ARG otherwise: the caller keeps the three launches). */
typedef struct {
    const void* df; const void* dg; const void* dh;         /* [npix][C/8], [npix][C/8], [npix][C] */
    const void* wf_pack; const void* wg_pack; const void* wh_pack;
    const void* add;                                        /* [npix][C] or NULL */
    const void* mask_b;                                     /* [npix][C] or NULL */
    void* dx;                                               /* [npix][C] */
    int64_t npix;
    int32_t C, accumulate;
} msau_attn_proj_bwd_args;
int msau_attn_proj_bwd(void* stream, int dtype, const msau_attn_proj_bwd_args* a);

/* The two data gradients of a 1x1 conv over concat(x1, x2) with 64 + 64 input channels (the coupling conv of a coupled stage at the
 * bottleneck level, model/model.py:143-148) as ONE launch -- the 64-channel counterpart of MSAU_CONV_DOUT, which the tile / row kernels
 * implement up to 32 + 32:
 *   dx1 = [mask1 > 0 ?] (W1^T g [+ dx1_old]),   dx2 = [mask2 > 0 ?] (W2^T g [+ dx2_old])
 * w1_pack / w2_pack: the packed data-gradient images of the two sources exactly as msau_conv2d takes them
 * (msau_conv_pack_geometry(dtype, 64, 0, 64, 1, 1, 1, 1, 1): one chunk, 64 rows, kchunk 64).  bf16, C = 64 only. */
typedef struct {
    const void* g;                                          /* [npix][C]: gradient of the conv's output (already masked by its ReLU) */
    const void* w1_pack; const void* w2_pack;
    void* dx1; void* dx2;                                   /* [npix][C] each */
    const void* mask1; const void* mask2;                   /* [npix][C] or NULL */
    int64_t npix;
    int32_t C, accumulate1, accumulate2, reserved;
} msau_dgrad2_args;
int msau_dgrad2_1x1(void* stream, int dtype, const msau_dgrad2_args* a);

/* ------------------------------------------------------------------------------------------
 * Masked cross entropy (model/model.py:446-459) with the batch rule of SURVEY 8(e):
 *   loss = scale * sum_b 1/max(cnt_b,1) * sum_{p: label!=0} -log softmax(logits_p)[label_p]
 *   dlogits = scale/cnt_b * (softmax - onehot) at labelled pixels, 0 elsewhere (and in padded channels)
 * counts: [B] int32 (written by msau_label_counts).  loss_accum: one float, += (deterministic:
 * per-block partials then one ordered pass).  ws: >= msau_ce_ws_floats(npix) floats.
 * ------------------------------------------------------------------------------------------ */
int msau_label_counts(void* stream, const int64_t* labels, int32_t* counts, int B, int64_t hw);
/* the same count with every sample spread over K workgroups: partial[b * K + k] (K <= 64) is written; msau_masked_ce_multi adds the
 * K integers of a sample up itself (counts_k = K) -- no atomics, no follow-up launch */
int msau_label_counts_split(void* stream, const int64_t* labels, int32_t* partial, int B, int64_t hw, int K);
int64_t msau_ce_ws_floats(int64_t npix_total);
int msau_masked_ce(void* stream, int dtype, const void* logits, const int64_t* labels, const int32_t* counts,
                   void* dlogits, float* loss_accum, float* ws, int B, int64_t hw, int C, int Cs, float scale);
/* final + auxiliary logits in one launch (model/model.py:455-458): loss[0] = CE(logits) + CE(aux) (aux may be NULL),
 * written, not accumulated; ws: msau_ce_multi_ws_floats(B*hw) floats of scratch.  Same arithmetic per pixel as
 * msau_masked_ce; the block sums are added in index order by a one-wave follow-up kernel.  counts_k = 1: counts is [B] as
 * msau_label_counts writes it; counts_k = K > 1: [B][K] partial counts of msau_label_counts_split (B <= 1024). */
int64_t msau_ce_multi_ws_floats(int64_t npix_total);
int msau_masked_ce_multi(void* stream, int dtype, const void* logits, const void* aux, const int64_t* labels,
                         const int32_t* counts, void* dlogits, void* daux, float* loss, float* ws,
                         int B, int64_t hw, int C, int Cs, float scale, int counts_k);

/* plain cross entropy over EVERY pixel (label 0 is a class), as model/training/cost.py:35-65 `UNetLoss`:
 *   loss += scale * sum_p -log softmax(logits_p)[label_p] ; dlogits = scale * (softmax - onehot)           */
int msau_softmax_ce(void* stream, int dtype, const void* logits, const int64_t* labels, void* dlogits,
                    float* loss_accum, float* ws, int B, int64_t hw, int C, int Cs, float scale);
/* the same with per-class weights, torch.nn.CrossEntropyLoss(weight) as `UNetLoss(class_weights=...)` builds it
 * (model/training/cost.py:24-31): class_w = float[C] on the device;
 *   sums[0] += sum_p w_p nll_p, sums[1] += sum_p w_p (w_p = class_w[label_p]);  dlogits = w_p (softmax - onehot)   -- UN-normalised:
 * the loss is sums[0] / sums[1] and the caller scales dlogits by 1 / sums[1] (known only after the pass). ws: msau_ce_ws_floats. */
int msau_softmax_ce_weighted(void* stream, int dtype, const void* logits, const int64_t* labels, const float* class_w,
                             void* dlogits, float* sums, float* ws, int B, int64_t hw, int C, int Cs);

/* ------------------------------------------------------------------------------------------
 * Global-norm clip + Adam on flat fp32 buffers (train_chargrid_funsd_msau.py:24-26,58-59).
 * state (device, 8 floats): [0]=step count, [1]=grad norm (after grad_scale), [2]=clip coef,
 *                           [3]=1-b1^t, [4]=1-b2^t.   step is incremented by the call.
 * grad_scale is applied to the gradient first (1/world after an all-reduce sum).
 * ------------------------------------------------------------------------------------------ */
int64_t msau_adam_ws_floats(int64_t n);
int msau_clip_adam_step(void* stream, float* params, const float* grads, float* m, float* v, float* state,
                        float* ws, int64_t n, float lr, float beta1, float beta2, float eps, float max_norm,
                        float grad_scale);

/* ------------------------------------------------------------------------------------------
 * The optimisers of the reference's get_optimizer (model/training/optimizer.py:4-31) as one fused multi-tensor step on the
 * flat fp32 buffers; torch.optim's arithmetic, element for element, with g = grads * grad_scale * clip_coef + weight_decay * p:
 *   MSAU_OPTIM_ADAM      m = c1 m + (1 - c1) g; v = c2 v + (1 - c2) g g; p -= lr / (1 - c1^t) * m / (sqrt(v) / sqrt(1 - c2^t) + eps)
 *                        (c1, c2 = beta1, beta2; state_a = exp_avg, state_b = exp_avg_sq: msau_clip_adam_step plus weight decay)
 *   MSAU_OPTIM_RMSPROP   s = c1 s + (1 - c1) g g; p -= lr g / (sqrt(s) + eps)        (c1 = alpha; state_a = square_avg; no momentum,
 *                        not centered)
 *   MSAU_OPTIM_MOMENTUM  b = c1 b + g; p -= lr b                                     (c1 = momentum; state_a = momentum_buffer; dampening 0,
 *                        no Nesterov; eps unused)
 * c1, c2 are doubles because torch forms 1 - c in double before it rounds to fp32 (1.f - 0.999f is off by 5e-5), and ADAM's bias
 * corrections 1 - c^t are taken in double as well.  state_b is NULL and c2 unused where the kind has no second buffer.  state: the 8 floats of msau_clip_adam_step, same slots
 * ([3], [4] are written under ADAM only); step is incremented by the call.
 * max_norm > 0: global-norm clip as msau_clip_adam_step (a sum-of-squares launch in a fixed order, then the update; state[1] and
 * state[2] are written); ADAM takes the two launches without clipping as well (coef 1).  max_norm <= 0 under RMSPROP / MOMENTUM:
 * ONE launch, state[1] / state[2] are left alone and ws may be NULL.  No floating-point atomics: equal inputs, equal bits.
 * skip: HOST array of n_skip <= MSAU_OPTIM_MAX_SKIP half-open element ranges [begin, end), ascending, not overlapping, inside
 * [0, n) (read during the call, passed to the kernel by value).  Parameters and state inside a range are left bit-unchanged --
 * no update, no weight decay: torch's treatment of a parameter whose gradient is None.  grads must be zero there.
 * ------------------------------------------------------------------------------------------ */
#define MSAU_OPTIM_ADAM 0
#define MSAU_OPTIM_RMSPROP 1
#define MSAU_OPTIM_MOMENTUM 2
#define MSAU_OPTIM_MAX_SKIP 8
int64_t msau_optim_ws_floats(int64_t n);
int msau_optim_step(void* stream, int kind, float* params, const float* grads, float* state_a, float* state_b, float* state,
                    float* ws, int64_t n, float lr, double c1, double c2, float eps, float weight_decay, float max_norm,
                    float grad_scale, const int64_t* skip, int n_skip);

/* ------------------------------------------------------------------------------------------
 * Chargrid rasteriser (next row N1; data_generator_funsd_bert.py:149-186 get_box_mask_box_label_word).
 * boxes: int32 [n][6] = {sample, y0, y1, x0, x1, value}, half-open, painted in order (later overwrites
 * earlier), clipped to the grid.  owner: int32 [B][H][W] scratch (index of the last covering box, -1).
 *   msau_raster_onehot : grid[b][y][x][c] = (c == value of the owning box); value < 0 paints zeros
 *   msau_raster_labels : labels[b][y][x]  = value of the owning box, 0 where none
 * ------------------------------------------------------------------------------------------ */
int msau_raster_owner(void* stream, const int32_t* boxes, int n, int32_t* owner, int B, int H, int W);
/* Ragged batch (documents of their own (h, w) at the origin of one H x W canvas): every box is in the coordinates of its own
 * document and is clipped at that DOCUMENT's edge -- what numpy slicing does on the reference's h x w array
 * (data_generator_funsd_bert.py:64-93) -- not at the canvas edge.  extent: int32 [B][2] = (h, w) of every sample (level 0 of a ragged
 * plan's extents; not NULL; values beyond the canvas are clipped to it).  owner is -1 everywhere outside the documents, so
 * msau_raster_onehot / _labels / _dense on it write zeros there, and MSAU_CONV_OWNER | MSAU_CONV_EXTENT gathers nothing there. */
int msau_raster_owner_ext(void* stream, const int32_t* boxes, int n, int32_t* owner, int B, int H, int W, const int32_t* extent);
int msau_raster_onehot(void* stream, int dtype, const int32_t* boxes, const int32_t* owner, void* grid_nhwc,
                       int B, int H, int W, int C, int Cs);
int msau_raster_labels(void* stream, const int32_t* boxes, const int32_t* owner, int64_t* labels, int B, int H, int W);
/* BERT-embedding chargrid (data_generator_funsd_bert.py:64-93 get_box_mask_box_label, :240): the owning box's feature
 * vector feats[value][0..C) (fp32 [n_vectors][C], device) at every covered pixel, zeros elsewhere. */
int msau_raster_dense(void* stream, int dtype, const int32_t* boxes, const int32_t* owner, const float* feats,
                      void* grid_nhwc, int B, int H, int W, int C, int Cs);

/* ------------------------------------------------------------------------------------------
 * Box convolution for the model/model_box.py variant (MultiBoxConvBlock, model_box.py:9-59: BoxConv2d(c, 3, 28, 28)
 * from the third-party package `box_convolution`, then a 1x1 conv).  PARITY UNPINNED: that package is absent and the
 * reference holds no fixtures for it; the arithmetic follows the published definition (Burkov & Lempitsky, NeurIPS
 * 2018) and is checked against oracle/box_oracle.py only.  Pixels are unit squares, zero outside the image:
 *   out[b,y,x,c*F+f] = 1/A * integral over rows [y+hmin, y+hmax+1) x columns [x+wmin, x+wmax+1) of in[b,.,.,c],
 *   A = (hmax-hmin+1)*(wmax-wmin+1), (hmin,hmax,wmin,wmax)[c][f] = stored parameter * max box size (real-valued).
 *   msau_box_integral  : NHWC `dtype` input -> fp32 integral image, channel-planar [B][C][H+1][W+1]
 *   msau_box_params    : stored parameters (four [C][F] tensors inside the flat fp32 parameter buffer, element offsets)
 *                        -> boxes in pixels fp32 [4][C][F], kept valid (|edge| <= max size, max >= min), and the
 *                        reflected boxes the input gradient uses
 *   msau_box_filter    : the box filter read from an integral image; sum_filters = 1: out[c] = sum over the F filters
 *                        (input gradient = msau_box_filter on the integral image of the output gradient with the
 *                        reflected boxes); accumulate = 1: added to `out`
 *   msau_box_param_grad: d loss / d stored parameters, written (not accumulated) into the flat fp32 gradient buffer;
 *                        ws: msau_box_pgrad_ws_floats() floats of scratch (per-workgroup partials, ordered final sum)
 * ------------------------------------------------------------------------------------------ */
int64_t msau_box_integral_ws_floats(int B, int H, int W, int C);      /* scratch of msau_box_integral (row-segment column sums) */
int msau_box_integral(void* stream, int dtype, const void* in_nhwc, float* ii, float* ws, int B, int H, int W, int C, int Cs, int relu_in);
int msau_box_params(void* stream, const float* flat_params, int64_t off_hmin, int64_t off_hmax, int64_t off_wmin, int64_t off_wmax,
                    int C, int F, float max_h, float max_w, float* params_fwd, float* params_refl);
/* sum_filters = 0: ii has C planes, out[c*F+f].  sum_filters = 1 (input gradient): ii has C*F planes (plane c*F+f is
 * filtered with box c*F+f), out[c] = sum over f.  Epilogue as msau_conv2d: v *= (mask_a > 0); v += add; v += out
 * (accumulate); v *= (mask_b > 0); the three operands share out's shape and may be NULL. */
int msau_box_filter(void* stream, int dtype, const float* ii, const float* params, void* out_nhwc, int B, int H, int W, int C, int F,
                    int Cs_out, int sum_filters, int accumulate, const void* mask_a, const void* add, const void* mask_b);
int64_t msau_box_pgrad_ws_floats(int B, int H, int W, int C, int F);
int msau_box_param_grad(void* stream, int dtype, const float* ii, const float* params, const void* gout_nhwc, float* ws, float* flat_grads,
                        int64_t off_hmin, int64_t off_hmax, int64_t off_wmin, int64_t off_wmax, int B, int H, int W, int C, int F,
                        int Cs_out, float max_h, float max_w);

/* one box conv inside a launch sequence (MSAU_OP_BOX_FWD / MSAU_OP_BOX_BWD):
 *   forward : ii = integral(ReLU?(in)); out = box_filter(ii, params_fwd)
 *   backward: box-parameter gradient (ii, gout) -> flat_grads; ii_g = integral(gout); gin = epilogue(box_filter(ii_g, params_refl, sum)) */
typedef struct {
    const void* in; float* ii; const float* params_fwd; const float* params_refl; void* out;
    const void* gout; void* gin; float* ii_g; float* ws; float* flat_grads; float* ws_ii;
    const void* mask_a; const void* add; const void* mask_b;
    int64_t off_hmin, off_hmax, off_wmin, off_wmax;
    int32_t B, H, W, C, F, Cs_in, Cs_out, relu_in, accumulate;
    float max_h, max_w;
} msau_box_args;
int msau_box_fwd(void* stream, int dtype, const msau_box_args* a);
int msau_box_bwd(void* stream, int dtype, const msau_box_args* a);

/* ------------------------------------------------------------------------------------------
 * Launch-sequence executor: one call enqueues a whole pre-built list of the launches above (the static
 * plan of a forward or backward sweep), so the host cost per launch is a switch, not a Python/ctypes
 * round trip.  `args` points to the msau_*_args / descriptor struct of the op's kind; all pointers
 * inside must stay valid until the call returns (they are read at enqueue time only).
 * ------------------------------------------------------------------------------------------ */
enum {
    MSAU_OP_CONV2D = 1,      /* args: msau_conv_desc          */
    MSAU_OP_WGRAD = 2,       /* args: msau_wgrad_desc         */
    MSAU_OP_LRN_FWD = 3,     /* args: msau_lrn_args           */
    MSAU_OP_LRN_BWD = 4,     /* args: msau_lrn_args           */
    MSAU_OP_POOL_FWD = 5,    /* args: msau_pool_args          */
    MSAU_OP_POOL_BWD = 6,    /* args: msau_pool_args          */
    MSAU_OP_ATTN_FWD = 7,    /* args: msau_attn_args          */
    MSAU_OP_ATTN_BWD = 8,    /* args: msau_attn_args          */
    MSAU_OP_CHANNEL_SUM = 9, /* args: msau_csum_args          */
    MSAU_OP_WGRAD_REDUCE = 10, /* args: msau_reduce_args      */
    MSAU_OP_CONV_PAIR = 11,  /* args: msau_conv_pair_desc     */
    MSAU_OP_BOX_FWD = 12,    /* args: msau_box_args           */
    MSAU_OP_BOX_BWD = 13,    /* args: msau_box_args           */
    MSAU_OP_ALLREDUCE = 14,  /* args: msau_allreduce_args     */
    MSAU_OP_ATTN_PROJ_BWD = 15, /* args: msau_attn_proj_bwd_args */
    MSAU_OP_DGRAD2_1X1 = 16  /* args: msau_dgrad2_args        */
};
typedef struct { int32_t kind; int32_t dtype; const void* args; } msau_op;
typedef struct { const void* a; const void* dy; void* out; int64_t npix; int32_t C, Cs, n; float alpha, beta, k; } msau_lrn_args;
/* extent (ABI v11): NULL, or the ragged batch's [B][2] (h, w) of the pool input grid (backward: msau_maxpool2x2_bwd_ext) / of the
 * attention's bottleneck grid, W columns wide (msau_selfattn_*_ext) */
typedef struct { const void* x_or_dy; void* y_or_dx; uint8_t* idx; const void* mask; int32_t B, H, W, Cs, accumulate;
                 const int32_t* extent; } msau_pool_args;
typedef struct { const void* f; const void* g; const void* h; const void* x_or_dy; void* y; float* stats;
                 void* df; void* dg; void* dh; float* ws; int32_t B, N, Ds, Cs; const int32_t* extent; int32_t W, reserved0; } msau_attn_args;
typedef struct { const void* g; int64_t npix; int32_t Cs; float* partials; int32_t nblk; } msau_csum_args;
typedef struct { const float* slab_arena; float* flat_grads; const msau_unpack_entry* table_dev; int32_t n_entries, max_elems; } msau_reduce_args;
typedef struct { void* comm; float* buf; int64_t count; } msau_allreduce_args;
int msau_run_ops(void* stream, const msau_op* ops, int n);
/* As msau_run_ops, but ops whose kind carries MSAU_OP_SIDE are enqueued on `side_stream` after everything
 * enqueued so far on `stream` (event fork); `stream` waits for `side_stream` at the end (join).  Used for
 * the weight gradients: they depend on a finished output gradient and feed nothing but the final slab
 * reduction, so they run beside the data-gradient chain. */
#define MSAU_OP_SIDE 0x100
int msau_run_ops_overlap(void* stream, void* side_stream, const msau_op* ops, int n, int join);   /* join=0: leave the side stream running */
/* Ops whose kind carries MSAU_OP_PROBE are bracketed by a pair of timing HIP events on the stream they are launched
 * on, inside the normal sequence (concurrent side-stream work included): the in-situ duration bench.py's roofline
 * object quotes.  msau_probe_read synchronises on the recorded events, writes up to `cap` durations in microseconds
 * in launch order, stores the count in *n and clears the list. */
/* An op carrying MSAU_OP_JOIN first makes `stream` wait for everything enqueued so far on `side_stream` (used by the
 * plan's deterministic mode: the level-0 LRN backward then never shares the device with a weight-gradient kernel). */
#define MSAU_OP_JOIN 0x800
#define MSAU_OP_PROBE 0x200
/* msau_run_ops_dp: as msau_run_ops_overlap, with a third stream for the gradient exchange.  An op carrying MSAU_OP_COMM
 * (MSAU_OP_ALLREDUCE records: one bucket of the flat gradient, placed behind the slab reduction that completes it) is
 * enqueued on `comm_stream` after everything enqueued so far on `side_stream` and on `stream`; the sweep goes on meanwhile.
 * With join != 0 `stream` finally waits for both other streams: the optimiser step may follow.  msau_run_ops runs such ops
 * in place on its one stream. */
#define MSAU_OP_COMM 0x400
int msau_run_ops_dp(void* stream, void* side_stream, void* comm_stream, const msau_op* ops, int n, int join);
int msau_probe_read(float* us, int cap, int* n);
/* cost of an event pair with nothing between its two records, averaged over `reps` pairs on `stream` (microseconds):
 * the part of a probed duration that is the probe itself */
int msau_probe_overhead(void* stream, int reps, float* us);

/* ------------------------------------------------------------------------------------------
 * Data-parallel gradient exchange (SURVEY 8b "msau_allreduce_bucket", 8e): one process per GPU, RCCL over xGMI.  The
 * reference has no distributed code; the exchange sits where a DDP hook would, between loss.backward() and
 * optimizer.step() (train_chargrid_funsd_msau.py:57-59).
 *   msau_comm_available   : 1 if librccl.so could be loaded (it is resolved at run time, not a link dependency)
 *   msau_comm_unique_id   : rank 0 draws the 128-byte id of a new communicator; ship it to the other ranks
 *   msau_comm_init        : collective -- every rank, with its device current, the same id; *comm_out is the handle
 *   msau_allreduce_bucket : in-place fp32 SUM over ranks of buf[0..count) on `stream`; asynchronous like a kernel launch
 * ------------------------------------------------------------------------------------------ */
int msau_comm_available(void);
int msau_comm_unique_id(void* id128_out, int bytes);
int msau_comm_init(void** comm_out, int world, int rank, const void* id128, int bytes);
int msau_comm_destroy(void* comm);
int msau_allreduce_bucket(void* stream, void* comm, float* buf, int64_t count);

/* context of an MSAU_CONV_OWNER launch (host struct; every pointer inside is a DEVICE pointer) */
typedef struct {
    const int32_t* owner;       /* [B][H][W]: index of the box that owns the pixel, -1 = none (msau_raster_owner)              */
    const int32_t* boxes;       /* [n_boxes][6] = sample, y0, y1, x0, x1, value (= row of feats)                               */
    const float* feats;         /* [n_vec][C] fp32 feature table                                                              */
    const float* w;             /* the conv's fp32 master weight, OIHW [8][C][3][3] (rounded to the storage type on the fly)   */
    float* wt;                  /* workspace, wt_floats >= 72 * roundup(C, 32) floats (the weight re-ordered and rounded for the table
                                   product: fp32 storage uses 72 * C floats, bf16 storage 80 * roundup(C, 32) bf16 values)          */
    float* table;               /* workspace, n_vec * 72 floats  (forward)                                                    */
    float* sums;                /* workspace, n_boxes * 72 floats (weight gradient)                                           */
    float* csum;                /* workspace, csum_blocks * 8 floats (bias gradient partials, msau_channel_sum)               */
    int32_t n_boxes, n_vec, C, csum_blocks;
    int32_t wt_floats;          /* floats the caller allocated behind `wt`: the launch refuses a workspace that is too small      */
    int32_t reserved0;
} msau_owner_ctx;

int msau_owner_slabs(const msau_wgrad_desc* d);   /* slabs an MSAU_CONV_OWNER weight gradient of this descriptor writes (<= d->nslabs) */

/* misc */
/* occupy the stream for ~microseconds (<= 200000) with a single sleeping wave: measurement aid only */
int msau_spin(void* stream, int microseconds);
int msau_fill_zero(void* stream, void* p, int64_t bytes);
/* stress check of what msau_run_ops_overlap's FORK events rest on (tests): `iters` rounds of [a kernel on `stream` rewrites `words`
 * 32-bit words, an event created with (system_fence = 1) or without (0: hipEventDisableSystemFence) the system-scope fence forks, a
 * kernel on `side_stream` counts the words that do not hold the new pattern, a default event joins]; *mismatches = that count, summed */
int msau_fork_visibility_check(void* stream, void* side_stream, int iters, int64_t words, int system_fence, int64_t* mismatches);
/* a non-blocking stream with queue priority -1 (device's highest), 0 (default) or +1 (device's lowest); the caller owns it */
int msau_stream_create(int priority, void** stream_out);
int msau_stream_destroy(void* stream);
int msau_softmax_channels_nchw(void* stream, const float* logits, float* pred, int B, int C, int64_t hw);

/* ------------------------------------------------------------------------------------------
 * Inference head and input painter (next row N2; inference/kv_model.py:274-276,305-313).
 *   msau_softmax_argmax_nhwc : probs[p][c] = softmax_c(logits[p][0..C)), argmax[p] = first maximum of probs[p];
 *                              logits [npix][Cs] in `dtype` storage, probs fp32 [npix][C] dense, argmax uint8 [npix]
 *                              (the stand-alone form of MSAU_CONV_HEAD, bit-identical to it; any C <= 255)
 *   msau_onehot_ids          : grid[p][c] = (c == ids[p]) for c < C, 0 for C <= c < Cs -- to_categorical() of the
 *                              character-id mask (generic_util.py:97-98) written straight into the NHWC input
 *   msau_onehot_ids_ext      : ragged batch: msau_onehot_ids inside every sample's extent, all-zero channels outside it
 *                              whatever the id there; ids [B][H][W], extent int32 [B][2] = (h, w) at level 0 (not NULL)
 *   msau_eval_confusion      : evaluation counts.  logits [B][H][W][Cs] in `dtype` storage (C real classes, C <= 64),
 *                              labels int64 [B][H][W].  A pixel counts when its label is in [1, C) and, with `extent` not
 *                              NULL, it lies inside its sample's extent; pred = index of the FIRST maximum of the C stored
 *                              values (as float: torch's argmax of the fp32 export, ties included), a 0 becomes zero_as
 *                              when zero_as >= 0; then counts[label * C + pred] += 1.  counts int64 [C][C] accumulates
 *                              across calls (zero it first); integer sums, independent of arrival order
 *   msau_box_vote            : entity-level predictions: every box of a list gets the class most of its pixels vote for.
 *                              logits as for msau_eval_confusion (1 <= C <= 64, C <= Cs, Cs % 8 == 0); boxes int32 [n][6] =
 *                              sample, y0, y1, x0, x1, value.  Box i is clipped as msau_raster_owner (extent NULL) or
 *                              msau_raster_owner_ext (extent int32 [B][2]) clip it; a sample outside [0, B) is an empty box.
 *                              A pixel's class is the first maximum of its C stored values (NaN counts as the maximum),
 *                              0 -> zero_as when zero_as >= 0.  owner NULL: the whole clipped rectangle votes; otherwise
 *                              owner int32 [B][H][W] is the map msau_raster_owner[_ext] wrote for this same list and only
 *                              the pixels with owner == i vote (every pixel votes for one box).
 *                              hist int32 [n][C] (may be NULL): votes per class, zeros included; votes int32 [n][2] = (votes
 *                              of the winner, voting pixels); pred int32 [n] = the smallest class among the most voted, -1
 *                              (and votes 0, 0) when no pixel votes.  counts int64 [C][C] (may be NULL) accumulates across
 *                              calls: counts[value * C + pred] += 1 for the boxes with 1 <= value < C and pred >= 0.
 *                              Every element of pred / votes / hist is written exactly once; all integers, independent of
 *                              arrival order.  n == 0 launches nothing; H * W < 2^31
 * ------------------------------------------------------------------------------------------ */
int msau_softmax_argmax_nhwc(void* stream, int dtype, const void* logits, float* probs, uint8_t* argmax,
                             int64_t npix, int C, int Cs);
int msau_onehot_ids(void* stream, int dtype, const int32_t* ids, void* grid_nhwc, int64_t npix, int C, int Cs);
int msau_onehot_ids_ext(void* stream, int dtype, const int32_t* ids, void* grid_nhwc, int B, int H, int W, int C, int Cs,
                        const int32_t* extent);
int msau_eval_confusion(void* stream, int dtype, const void* logits, const int64_t* labels, int64_t* counts, int B, int H, int W,
                        int C, int Cs, int zero_as, const int32_t* extent);
int msau_box_vote(void* stream, int dtype, const void* logits, const int32_t* boxes, int n, const int32_t* owner, int32_t* pred,
                  int32_t* votes, int32_t* hist, int64_t* counts, int B, int H, int W, int C, int Cs, int zero_as,
                  const int32_t* extent);

/* ------------------------------------------------------------------------------------------
 * Region extraction for key-value inference (the per-pixel part of inference/kv_model.py:150-261), one workgroup per
 * (document, class c in [2, n_class)), the document in LDS.
 *   msau_kv_regions_limits : out int32 [6] = (pixels a document may have, regions per (document, class), pairs per (document,
 *                            class), int32 per region record, int32 per pair record, lines per document)
 *   msau_kv_regions        : argmax uint8 [B][H][W] (the head's class map), line_ids / char_pos uint16 [B][H][W], boxes int32 [n][4] =
 *                            (x1, y1, x2, y2) of every document's lines in grid coordinates, box_off int32 [B + 1] (document b owns
 *                            boxes[box_off[b] .. box_off[b + 1]); line id v means box v - 1 of its document), extent int32 [B][2] =
 *                            (h, w) or NULL for a dense batch (h, w = H, W).  All device memory.  Per class: M = closing of
 *                            (argmax == c) with a 1 x 3 element, zero outside the document; its 4-connected components in
 *                            raster order of their first pixel.
 *                              header  int32 [B][n_class][4]: row c >= 2 = (region offset, regions, pair offset, pairs) of class c
 *                                      inside the document's slices; row 0 = (region cursor, pair cursor, 0, 0); zeroed here
 *                              regions int32 [B][cap_regions][8] = (first_y, first_x, y0, y1, x0, x1, pixels, c), box half-open
 *                              pairs   int32 [B][cap_pairs][4]   = ((k << 16) | v, n_under, cp_min, cp_max) sorted by the key:
 *                                      n_under = pixels of component k with line id v, cp_min / cp_max = extremes of the non-zero
 *                                      char_pos under k inside box v - 1 clipped to the document (65535 / 0 when there is none)
 *                              overflow int32 [B], zeroed here: 1 the document has more pixels than the LDS form holds (or its
 *                                      extent is outside the canvas), 2 the labelling did not converge within its bound,
 *                                      4 more regions / 8 more pairs than a table or the document's slice holds, 16 a line id
 *                                      beyond the document's boxes.  A flagged document's rows are to be ignored; the others'
 *                                      are complete.  Integers only, independent of arrival order but for the slice offsets.
 * ------------------------------------------------------------------------------------------ */
int msau_kv_regions_limits(int32_t* out);
int msau_kv_regions(void* stream, const uint8_t* argmax, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes,
                    const int32_t* box_off, const int32_t* extent, int B, int H, int W, int n_class, int32_t* header,
                    int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int32_t* overflow);
/*   msau_kv_regions_large  : the same table for documents of any size (h * w < 2^31): the same phases with the labels in a
 *                            workspace in device memory, one workgroup per (listed document, class), each on its own h * w int32
 *                            of it.  To be called after msau_kv_regions, on the same stream, with the same arguments and output
 *                            buffers, for the documents that launch flagged 1 (the caller knows them from their sizes).
 *                              docs    int32 [n_docs] in HOST memory: the documents to redo, each in [0, B), none twice
 *                              ws_off  int64 [n_docs] in HOST memory, increasing: document docs[i] owns workspace[ws_off[i] ..
 *                                      ws_off[i + 1]) (the last one up to workspace_ints) and needs (n_class - 2) * h * w of it
 *                              workspace int32 [workspace_ints] in device memory; holds nothing between calls
 *                            For each listed document: its overflow word is REPLACED by this launch's own flags (1: h * w or
 *                            the extent out of range, or its workspace share too small; 2 .. 16 as above), its header rows are
 *                            zeroed and written, its list slices written.  No other document is touched.  The limits per class
 *                            (msau_kv_regions_limits) and the capacities hold as above. */
int msau_kv_regions_large(void* stream, const uint8_t* argmax, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes,
                          const int32_t* box_off, const int32_t* extent, int B, int H, int W, int n_class, const int32_t* docs,
                          int n_docs, const int64_t* ws_off, int32_t* workspace, int64_t workspace_ints, int32_t* header,
                          int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int32_t* overflow);
/*   msau_kv_regions_scored, msau_kv_regions_large_scored : the two calls above with a confidence per region.  Everything they
 *                            write they write as above (header, regions, pairs and overflow are the same words), plus
 *                              probs   fp32 [B][H][W][n_class] on the canvas: the head's probabilities (head_probs), read as stored
 *                              scores  int64 [B][cap_regions]: row r of document b belongs to the region record in row r of
 *                                      `regions`: the sum over the region's pixels (those of the closed mask, so the gap pixels
 *                                      the closing added count with the probability they have) of q(p) = rint(p * 65536), p =
 *                                      probs[b][y][x][c] of the region's class c, rounded to nearest even (the product by 2^16 is
 *                                      exact).  The mean probability of the region is scores / (65536 * pixels).  An integer
 *                                      sum, independent of arrival order: at most 24 576 * 65 536 < 2^31 in the LDS form, up to
 *                                      2^47 in the large form, summed in 64 bits in both.  Every row a class reserves is written,
 *                                      no other row is touched; a flagged document's rows are to be ignored.
 *                            NULL probs or scores are refused (MSAU_ERR_ARG). */
int msau_kv_regions_scored(void* stream, const uint8_t* argmax, const float* probs, const uint16_t* line_ids, const uint16_t* char_pos,
                           const int32_t* boxes, const int32_t* box_off, const int32_t* extent, int B, int H, int W, int n_class,
                           int32_t* header, int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int64_t* scores,
                           int32_t* overflow);
int msau_kv_regions_large_scored(void* stream, const uint8_t* argmax, const float* probs, const uint16_t* line_ids, const uint16_t* char_pos,
                                 const int32_t* boxes, const int32_t* box_off, const int32_t* extent, int B, int H, int W, int n_class,
                                 const int32_t* docs, int n_docs, const int64_t* ws_off, int32_t* workspace, int64_t workspace_ints,
                                 int32_t* header, int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int64_t* scores,
                                 int32_t* overflow);

/* ------------------------------------------------------------------------------------------
 * Mask painter for key-value inference (inference/kv_model.py:83-148 `_generate_masks_from_label`, the per-pixel part):
 * the three canvases the forward and msau_kv_regions read, painted from the documents' glyph tables
 * (msau_amd/inference/glyphs.py) in one launch.  Every canvas pixel is written, so nothing has to be cleared before.
 *   msau_kv_paint : lines int32 [n][8] = (x1, y1, x2, y2, first glyph, glyphs, xl, xr) per text line in document order: the box in
 *                   grid coordinates, its glyphs glyphs[first .. first + glyphs) counted from the document's first glyph, and the
 *                   columns [xl, xr) that the box and the glyph spans reach; glyphs = 0 is a line without text, which paints
 *                   nothing.  glyphs [m] of 8 bytes = (int16 a, int16 b, uint16 token, uint16 0): character k of its line covers
 *                   the columns [a, b); within a line the spans are disjoint and their starts increase (a_k <= b_k <= a_k+1, a_k < a_k+1).
 *                   line_off / glyph_off int32 [B + 1]: document b owns lines[line_off[b] .. line_off[b + 1]) and
 *                   glyphs[glyph_off[b] .. glyph_off[b + 1]); sizes int32 [B][2] = (h, w) <= (H, W).  All device memory, the
 *                   canvases 16-byte aligned.  Pixel (y, x) of document b:
 *                     line_ids = li + 1 of the LAST line li with text, y1 <= y < y2, and x1 <= x < x2 or x in one of its spans
 *                     ids / char_pos = token / k + 1 of glyph k of the LAST line with y1 <= y < y2 that has a span holding x
 *                     0 where there is none; outside the document ids = -1 and both masks 0 (ragged.pack_ids / pack_masks)
 *                   ids int32 [B][H][W], line_ids / char_pos uint16 [B][H][W].  Integers only, no atomics, no pixel limit.
 * ------------------------------------------------------------------------------------------ */
int msau_kv_paint(void* stream, const int32_t* lines, const void* glyphs, const int32_t* line_off, const int32_t* glyph_off,
                  const int32_t* sizes, int B, int H, int W, int32_t* ids, uint16_t* line_ids, uint16_t* char_pos);

/* ------------------------------------------------------------------------------------------
 * Key-value training (data_generator/data_generator_text.py:160-250, its affine and rotation warps (:303-344) as
 * msau_kv_warp_train below, model/training/cost.py:35-65 `UNetLoss`).
 *   msau_kv_paint_train : the painter of a training batch from the documents' training tables (msau_amd/training/kv_data.py): lines,
 *                   glyphs, offsets and sizes as msau_kv_paint takes them, line_labels int32 [n][2] = (label, aux label) per line, sharing
 *                   the lines' offsets.  ids int32 as msau_kv_paint writes them; labels / aux_labels int64 [B][H][W]: the record of
 *                   the LAST line with text whose box holds the pixel (y1 <= y < y2, x1 <= x < x2; the glyph spans play no part), 0
 *                   where there is none, -1 outside the document (ids -1 there too).  Every canvas pixel is written.
 *   msau_label_hist : partial[(b * K + k) * C + c] int32 = the pixels with label c in part k of K of document b, counted inside the
 *                   extent (h_b, w_b) (extent NULL: the whole H x W) among labels in [0, C); written, no atomics in global memory;
 *                   the K rows of a document add up to its class histogram.  C <= 256, K <= 64.
 *   msau_unet_ce  : UNetLoss and its gradient for B documents on one canvas, both heads in one launch, each head with its own
 *                   labels.  For document b with extent (h_b, w_b) (NULL: (H, W)) and class weights cw (NULL: all ones):
 *                     L_b(head) = sum_p cw[t_p] * nll_p / D_b(head),  D_b = sum_p cw[t_p]  over pixels inside the extent with t_p in [0, C)
 *                     loss3[0] = (1/B) sum_b (0.5 L_b(final) + 0.5 L_b(aux))      (aux NULL: L_b(final) alone)
 *                     loss3[1] = (1/B) sum_b L_b(final),  loss3[2] = (1/B) sum_b L_b(aux)   (aux NULL: 0)
 *                     dlogits  = head_weight / (B * D_b) * cw[t_p] * (softmax - onehot),  head_weight 0.5 (aux NULL: 1)
 *                   and 0 outside the extent, at labels outside [0, C) and in padded channels.  Without weights D_b is the extent's
 *                   area; with weights it is sum_c cw[c] * hist[b][c], classes in index order, hist the K rows of msau_label_hist
 *                   added up: hist_partial holds [B][K][C] of `labels`, then [B][K][C] of `aux_labels` when aux is given.  A
 *                   document with D_b = 0 contributes nothing.  loss3 is written; the block partials in ws
 *                   (>= msau_unet_ce_ws_floats(B*H*W) floats) are added in index order, so the three values are reproducible.
 *                   B <= 1024, B*H*W < 2^31; Cs <= 32 keeps a pixel's logits in registers.
 * ------------------------------------------------------------------------------------------ */
int msau_kv_paint_train(void* stream, const int32_t* lines, const void* glyphs, const int32_t* line_labels, const int32_t* line_off,
                        const int32_t* glyph_off, const int32_t* sizes, int B, int H, int W, int32_t* ids, int64_t* labels,
                        int64_t* aux_labels);
int msau_label_hist(void* stream, const int64_t* labels, const int32_t* extent, int32_t* partial, int B, int H, int W, int C, int K);
int64_t msau_unet_ce_ws_floats(int64_t npix_total);
int msau_unet_ce(void* stream, int dtype, const void* logits, const void* aux, const int64_t* labels, const int64_t* aux_labels,
                 const int32_t* extent, const float* class_w, const int32_t* hist_partial, int K, void* dlogits, void* daux,
                 float* loss3, float* ws, int B, int H, int W, int C, int Cs);

/* ------------------------------------------------------------------------------------------
 * Key-value validation (model/training/trainer.py's epoch print: UNetLoss and cost.py:44-48's accuracy, forward only).
 *   msau_unet_eval : per document, both heads in one launch, no gradient.  logits / aux / labels / aux_labels / extent / class_w
 *                   exactly as msau_unet_ce takes them (aux NULL: one head; extent NULL: (H, W); class_w NULL: all ones).
 *                     doc_loss   fp32  [B][2]    : [b][t] = L_b(head t) as defined for msau_unet_ce, 0 when D_b = 0
 *                     doc_counts int32 [B][2][2] : [b][t] = (labelled, correct): the pixels inside the extent whose label is in
 *                                                  [1, C), and those of them whose prediction equals the label; the prediction is
 *                                                  the index of the FIRST maximum of the C stored values read as float (the rule
 *                                                  of msau_eval_confusion: torch.argmax of the fp32 export)
 *                   head 1's entries are 0 when aux is NULL.  Every entry is written, nothing accumulates.  K in [1, 256] workgroups
 *                   per document each take ceil(h_b / K) rows of the extent and write one partial row into ws
 *                   (>= msau_unet_eval_ws_bytes(B, K) bytes, 16-byte aligned); a second launch adds a document's K rows in index
 *                   order and divides, so equal K gives equal bits.  The weighted denominator D_b is summed here, pixel by pixel:
 *                   no msau_label_hist launch.  Nothing outside the extents is read.  No floating-point atomics.
 *                   B <= 1024, B*H*W < 2^31, C <= Cs <= 256, Cs % 8 == 0; Cs <= 32 keeps a pixel's logits in registers.
 * ------------------------------------------------------------------------------------------ */
int64_t msau_unet_eval_ws_bytes(int B, int K);
int msau_unet_eval(void* stream, int dtype, const void* logits, const void* aux, const int64_t* labels, const int64_t* aux_labels,
                   const int32_t* extent, const float* class_w, int K, float* doc_loss, int32_t* doc_counts, void* ws, int B, int H,
                   int W, int C, int Cs);

/* ------------------------------------------------------------------------------------------
 * UNetLoss under another cost: the focal loss and the soft Dice loss beside the cross entropy, for training
 * (msau_unet_cost: the argument list of msau_unet_ce behind `kind, param`) and for validation (msau_unet_cost_eval: that of
 * msau_unet_eval).  Active pixels, extents, heads, class weights v = cw, loss3 / doc_loss / doc_counts and the gradient's zeros are
 * those of msau_unet_ce / msau_unet_eval; p = softmax over the C classes, y the label, p_t = p[y], nll = -log p_t.
 *   MSAU_COST_CE    : param unread; the bits of msau_unet_ce / msau_unet_eval (they are called).
 *   MSAU_COST_FOCAL : param = gamma >= 0.  L_b = sum_p v_y (1 - p_t)^gamma nll / D_b, D_b the cross entropy's denominator;
 *                     dlogits = CE's times m = (1 - p_t)^gamma + gamma p_t (1 - p_t)^(gamma - 1) nll.  gamma = 0 gives the CE bits;
 *                     where 1 - p_t rounds to 0 (gamma > 0) the pixel has loss 0 and gradient 0.  One launch of msau_unet_ce's
 *                     shape and its finish; ws as msau_unet_ce's.
 *   MSAU_COST_DICE  : param = smooth eps > 0.  Per document and class over the active pixels I_c = sum p_c [y = c], P_c = sum p_c,
 *                     Y_c = sum [y = c];  L_b = 1 - sum_c v_c (2 I_c + eps) / (P_c + Y_c + eps) / V,  V = sum_c v_c (L_b = 0 when
 *                     V = 0); every class counts.  dlogits[j] = head_weight / B * p_j (a_j - sum_c a_c p_c), a_c = hit_c at c = y,
 *                     else miss_c;  miss_c = (v_c / V)(2 I_c + eps) / den_c^2,  hit_c = miss_c - (v_c / V) 2 / den_c.
 *                     Training ALWAYS takes hist_partial (Y_c: the K rows of msau_label_hist per head, as for class weights) and
 *                     runs a K x B reduction that writes per-slab (I, P) rows, a coefficient step (the rows in index order) with
 *                     msau_unet_ce's finish, and a gradient pass of msau_unet_ce's shape that reads the (hit, miss) table from
 *                     global memory.  Validation takes its own histograms (min(K, 64) rows) into ws.
 * No floating-point atomics, every output written, every summation order fixed: equal arguments give equal bits.
 * msau_unet_cost_ws_floats: floats of ws for msau_unet_cost (Dice: for any K <= 64); msau_unet_cost_eval_ws_bytes: bytes of ws for
 * msau_unet_cost_eval.  An unknown kind, a gamma that is negative or not finite, a smooth that is not positive and finite, and Dice
 * training without hist_partial are MSAU_ERR_ARG before anything is launched.
 * ------------------------------------------------------------------------------------------ */
#define MSAU_COST_CE 0
#define MSAU_COST_FOCAL 1
#define MSAU_COST_DICE 2
int64_t msau_unet_cost_ws_floats(int kind, int B, int H, int W, int C);
int msau_unet_cost(void* stream, int dtype, int kind, float param, const void* logits, const void* aux, const int64_t* labels,
                   const int64_t* aux_labels, const int32_t* extent, const float* class_w, const int32_t* hist_partial, int K,
                   void* dlogits, void* daux, float* loss3, float* ws, int B, int H, int W, int C, int Cs);
int64_t msau_unet_cost_eval_ws_bytes(int kind, int B, int K, int C);
int msau_unet_cost_eval(void* stream, int dtype, int kind, float param, const void* logits, const void* aux, const int64_t* labels,
                        const int64_t* aux_labels, const int32_t* extent, const float* class_w, int K, float* doc_loss,
                        int32_t* doc_counts, void* ws, int B, int H, int W, int C, int Cs);

/* ------------------------------------------------------------------------------------------
 * The masked cost: the masked cross entropy of msau_masked_ce_multi -- the loss of TrainEngine.step and
 * MSAUWrapper.loss -- with class weights and under the costs above.  Both heads are scored against ONE label map; the active pixels
 * A_b of document b lie inside its extent (extent [B][2] = (h, w), NULL: the whole canvas) and have a label in [1, C): label 0, a
 * negative label and a label >= C are inactive.  v = class_w (NULL: ones), p / p_t / nll as above.
 *   MSAU_COST_CE    : L_b = sum_{A_b} v_y nll / D_b,  D_b = sum_{A_b} v_y (without weights: the number of labelled pixels); param unread.
 *   MSAU_COST_FOCAL : L_b = sum_{A_b} v_y (1 - p_t)^gamma nll / D_b;  gamma = 0 gives MSAU_COST_CE's bits.
 *   MSAU_COST_DICE  : the Dice formulas above with I_c, P_c, Y_c over A_b; all C classes count and Y_0 = 0.
 * loss3 = (mean_b (L_b(final) + L_b(aux)), mean_b L_b(final), mean_b L_b(aux)): head weights 1 and 1; aux NULL: one head, loss3[2] = 0,
 * daux untouched.  A document without an active pixel, with D_b = 0 or with V = 0 has loss 0 and gradient 0, and B still divides.
 * dlogits / daux: every stored channel of every pixel is written, exactly 0 at inactive pixels, outside the extents and in the
 * padded channels.  The kernels are msau_unet_cost's, compiled for one label map (read once per pixel for both heads), first
 * active class 1 and head weight 1; heads of up to 32 stored channels keep a pixel in registers, wider ones read it from the cache,
 * with equal bits.  No floating-point atomics, no memset, every summation order fixed.
 * hist_partial / K: msau_label_hist's rows of `labels` (1 <= K <= 64).  Dice and class weights need them (MSAU_ERR_ARG without);
 * the unweighted cross entropy and focal loss take them when given, and otherwise this call takes a histogram of its own into ws.
 * msau_masked_cost_eval: forward only, per document: doc_loss[b][t] = L_b(head t), doc_counts[b][t] = (labelled, correct) as
 * msau_unet_eval counts them; K workgroups per document (1 <= K <= 256); Dice takes its own histogram (min(K, 64) rows) into ws.
 * msau_masked_cost_ws_floats = msau_unet_ce_ws_floats(B*H*W) + 16 B C (CE, focal) or 2 B + 4 B C + 256 B C (Dice);
 * msau_masked_cost_eval_ws_bytes = msau_unet_eval_ws_bytes(B, K), for Dice + 4 (4 B K C + B min(K, 64) C).
 * Every argument error is MSAU_ERR_ARG before anything is launched.
 * ------------------------------------------------------------------------------------------ */
int64_t msau_masked_cost_ws_floats(int kind, int B, int H, int W, int C);
int msau_masked_cost(void* stream, int dtype, int kind, float param, const void* logits, const void* aux, const int64_t* labels,
                     const int32_t* extent, const float* class_w, const int32_t* hist_partial, int K,
                     void* dlogits, void* daux, float* loss3, float* ws, int B, int H, int W, int C, int Cs);
int64_t msau_masked_cost_eval_ws_bytes(int kind, int B, int K, int C);
int msau_masked_cost_eval(void* stream, int dtype, int kind, float param, const void* logits, const void* aux, const int64_t* labels,
                          const int32_t* extent, const float* class_w, int K, float* doc_loss,
                          int32_t* doc_counts, void* ws, int B, int H, int W, int C, int Cs);

/* ------------------------------------------------------------------------------------------
 * Key-value training, the generator's affine / rotation augmentation (data_generator/data_generator_text.py:303-344,
 * utils/image_util.py:38-55; msau_amd/training/kv_warp.py states what is computed, csrc/warp.hip how).
 *   msau_kv_warp_train : the canvases msau_kv_paint_train leaves (ids int32, labels / aux_labels int64 [B][H][W], src_sizes int32
 *                   [B][2] = (h, w) <= (H, W)) resampled as scipy's cubic spline resamples the generator's one-hot planes x 255
 *                   (order 3, mode "constant", cval 0), thresholded at > 64.  warps double [B][6] = m00, m01, m10, m11, off0, off1:
 *                   output pixel (oy, ox) of document b reads the source at off + M (oy, ox), (row, col) order, float64;
 *                   dst_sizes int32 [B][2] = (ho, wo) <= (Ho, Wo).  All device memory.
 *                     grid [B][Ho][Wo][Cs] in `dtype` (the plan's input): channel c < n_token is 1 iff the warped plane
 *                       [ids == c] exceeds the threshold -- multi-hot or zero-hot -- every other element 0: the channels from
 *                       n_token on, pixels whose source lies outside [0, h-1] x [0, w-1], outside (ho, wo) and in the padding
 *                     labels_out / aux_out int64 [B][Ho][Wo]: 1 if the warped plane [labels == 1] is set, else the smallest set
 *                       plane in [2, n_class), else 0; -1 outside (ho, wo)
 *                     flags int32 [B]: 0, or why the document has to be warped on the host instead (bit 0: more than 4 planes of
 *                       a pixel are set, or a pixel's 12 x 12 centre window holds more than 48 distinct values; bit 1: its matrix or
 *                       offset is not finite, nothing of it was resampled)
 *                   Every element of the four outputs is written exactly once, nothing is cleared first, no atomics: equal inputs
 *                   give equal bits.  Coordinates in float64 (no fused multiply-add), weights and sums in fp32 over a window of
 *                   32 x 32 source pixels: a plane's grey level is within 1e-4 + fp32 rounding of the float64 value, so the
 *                   outputs equal the float64 statement except where a plane comes that close to 64.5.  ws: int32
 *                   [msau_kv_warp_train_ws_ints(B, Ho, Wo)], one word per 16 x 16 tile.  Two launches (the tiles; the flags).
 *                   B <= 65535, B*H*W < 2^31, B*Ho*Wo < 2^31, n_token <= Cs, Cs % 8 == 0, n_token and n_class <= 32767, grid 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int64_t msau_kv_warp_train_ws_ints(int B, int Ho, int Wo);
int msau_kv_warp_train(void* stream, int dtype, const int32_t* ids, const int64_t* labels, const int64_t* aux_labels,
                       const int32_t* src_sizes, const double* warps, const int32_t* dst_sizes, int B, int H, int W, int Ho, int Wo,
                       int n_token, int Cs, int n_class, void* grid, int64_t* labels_out, int64_t* aux_out, int32_t* flags,
                       int32_t* ws);

/* ------------------------------------------------------------------------------------------
 * Key-value training, the generator's elastic augmentation (data_generator/data_generator_text.py:309-344,
 * utils/image_util.py:58-90; msau_amd/training/kv_warp.py "the elastic warp" states what is computed, csrc/warp.hip how).
 *   msau_kv_elastic_train : the canvases msau_kv_paint_train leaves (as for msau_kv_warp_train) resampled as scipy's
 *                   map_coordinates(order=1, mode "constant", cval 0) resamples the generator's one-hot planes x 255, thresholded
 *                   at > 64 after scipy's uint8 rounding.  fields uint8 [B][H][W][2] = (fy, fx) on the source canvas, alphas double
 *                   [B][2] = (alpha_y, alpha_x): output pixel (oy, ox) of document b reads the source at
 *                   (oy + fy * alpha_y, ox + fx * alpha_x), float64, the product rounded, then the sum.  A document's output
 *                   extent is its source size (h, w), clipped to (Ho, Wo).  All device memory.
 *                     grid [B][Ho][Wo][Cs] in `dtype`: channel c < n_token is 1 iff the bilinear grey level of the plane
 *                       [ids == c], (1-uy)((1-ux) p00 + ux p01) + uy((1-ux) p10 + ux p11) in float64 in this order, is >= 64.5 --
 *                       at most three channels of a pixel -- every other element 0: the channels from n_token on, pixels whose
 *                       source lies outside [0, h-1] x [0, w-1], outside (h, w) and in the padding
 *                     labels_out / aux_out int64 [B][Ho][Wo]: 1 if the plane [labels == 1] is set, else the smallest set plane in
 *                       [2, n_class), else 0; -1 outside (h, w)
 *                     flags int32 [B]: 0, or bit 1: an alpha of the document is not finite, nothing of it was resampled (zeros
 *                       and 0 labels inside its extent); bit 0 cannot occur
 *                   Every element of the four outputs is written exactly once, nothing is cleared first, no atomics: equal inputs
 *                   give equal bits.  Everything a pixel's planes depend on is float64 with no fused multiply-add, so the outputs
 *                   equal the float64 statement (`kv_warp.elastic_host`) bit for bit.  A tap never leaves the document: floor + 1
 *                   is clamped to n - 1, where its weight is 0.  Negative alphas are legal.  ws: int32
 *                   [msau_kv_elastic_train_ws_ints(B, Ho, Wo)], one word per 16 x 16 tile.  Two launches (the tiles; the flags).
 *                   B <= 65535, B*H*W < 2^31, B*Ho*Wo < 2^31, n_token <= Cs, Cs % 8 == 0, n_token and n_class <= 32767, grid 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int64_t msau_kv_elastic_train_ws_ints(int B, int Ho, int Wo);
int msau_kv_elastic_train(void* stream, int dtype, const int32_t* ids, const int64_t* labels, const int64_t* aux_labels,
                          const int32_t* src_sizes, const uint8_t* fields, const double* alphas, int B, int H, int W, int Ho, int Wo,
                          int n_token, int Cs, int n_class, void* grid, int64_t* labels_out, int64_t* aux_out, int32_t* flags,
                          int32_t* ws);

#ifdef __cplusplus
}
#endif
#endif /* MSAU_HIP_H */
