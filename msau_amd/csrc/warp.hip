// The generator's affine / rotation augmentation of a key-value training batch (data_generator/data_generator_text.py:303-344,
// utils/image_util.py:38-55), resampled from the painter's canvases: msau_kv_warp_train.  The generator warps n_token + 2 n_class
// one-hot planes x 255 with scipy's cubic spline (order 3, mode "constant"), thresholds each at > 64 and reads a label off each
// target; per plane that is (msau_amd/training/kv_warp.py, DESIGN.md 5e "Warps")
//   (sy, sx) = off + M (oy, ox) in float64; outside [0, h-1] x [0, w-1] every plane is 0
//   S_c = sum_{j,i} gy(j) gx(i) [canvas(j, i) == c],   g(p) = sum_{t=-1..2} beta3(s - f - t) * sqrt(3) z^|f + t - p|,  f = floor(s),
//   z = sqrt(3) - 2: the four B-spline taps times the mirror-boundary prefilter, positions outside [0, n-1] reflected by whole-sample
//   mirror; plane c is set iff 255 S_c > 64.5
// so the multi-hot input and both label maps come from the id canvas and the two label canvases and no one-hot plane ever exists.
//
// THE WINDOW.  g is summed over p = f-15 .. f+16 (WP_LO .. WP_HI: 32 positions per axis, 1024 per pixel).  Every dropped term has
// |f + t - p| >= 15, so the dropped L1 mass per axis is at most 2 sqrt(3) |z|^15 / (1 - |z|) = 1.25e-8, the L1 mass of g per axis is
// at most sqrt(3) (1 + |z|) / (1 - |z|) = 3, and a plane's grey level moves by at most 255 * 2 * 3 * 1.25e-8 = 1.9e-5 < 1e-4.
//
// NO ACCUMULATOR PER TOKEN.  A lane owns one output pixel and never keeps a sum per id.  A plane that is set must show in the CENTRE
// of the window (p = f-5 .. f+6 on both axes, WP_CLO .. WP_CHI): outside it the L1 mass per axis is at most
// 2 sqrt(3) |z|^5 / (1 - |z|) = 0.00654, so an id whose centre sum is P has |S - P| <= 2 * 3 * 0.00654 = 0.0392, and P <= 0.2
// (WP_CENTRE_MIN) means S <= 0.2392 < 64.5 / 255 = 0.2529.  The lane collects the distinct values of the 144 centre positions in
// its list in LDS (WP_CAND = 48 entries), keeps those whose centre sum (144 terms) passes, and of these the ones whose whole sum
// (1024 terms) passes: three loops, each over the lane's own list, so the lanes of a wavefront take their k-th candidates together
// instead of waiting for each other's.  The set ids of a pixel go to WP_MAXSET = 4 slots; a fifth, or a 49th distinct value in a
// centre, sets the document's flag (the caller warps that document on the host).  A label is 1 if plane 1 is set, else the smallest
// set plane >= 2, else 0.  Along a row g is geometric on both sides of the taps (g(d - 1) = z g(d) for d <= -1, g(d + 1) = z g(d)
// for d >= 2), so the inner loops multiply by z instead of looking weights up.
//
// One workgroup per 16 x 16 tile of one document's output.  The source pixels its windows can touch (the corners' coordinates, the
// window, and what the mirror folds back in) are staged in LDS as int16 (a value outside [0, 32766] can be no token and no class
// and is staged as -1: n_token, n_class <= 32767) when they fit WP_SRC x WP_SRC (a 16 x 16 tile under a
// rotation by 45 degrees needs 55 x 55); a tile of a map that stretches further reads the canvases directly.  Phases: stage ->
// one pixel per lane (labels stored, set ids left in LDS) -> the tile's channels stored 8 at a time, consecutive lanes consecutive
// addresses.  Every element of the three outputs is written exactly once, by exactly one lane; nothing is cleared, no atomics:
// equal inputs give equal bits.  A tile's flag goes to its own word of the workspace and a second launch folds a document's words
// into its flag.  Coordinates are float64 with the products and sums rounded one by one (no fused multiply-add: the in-range test
// has to agree with the host's to the bit); weights and sums are fp32.
//
// With -DMSAU_WARP_CPU the same phases compile as plain C++ and the lanes of a phase run one after another
// (tests/test_kv_warp_cpu.py; build it with -ffp-contract=off).
#ifdef MSAU_WARP_CPU
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#define WP_DEV static inline
#define WP_TABLE static const
#define WP_PHASE(fn) do { for (int t__ = 0; t__ < WP_THREADS; ++t__) fn(c, s, t__); } while (0)
#else
#include "msau_common.h"
#define WP_DEV __device__ __forceinline__
#define WP_TABLE __device__ const
#define WP_PHASE(fn) do { fn(c, s, (int)threadIdx.x); __syncthreads(); } while (0)
#endif

#define WP_THREADS 256
#define WP_TILE 16                  // output pixels per side of a tile: WP_TILE * WP_TILE == WP_THREADS
#define WP_LO (-15)                 // the window, as offsets from floor(s)
#define WP_HI 16
#define WP_CLO (-5)                 // its centre
#define WP_CHI 6
#define WP_CENTRE_MIN 0.2f
#define WP_SRC 64                   // side of the source tile in LDS
#define WP_MAXSET 4
#define WP_CAND 48                  // distinct values of a centre that a lane can list
#define WP_VALUE_MAX 32766
#define WP_FOLD_STEPS 36            // a window position is at most 16 outside [0, n-1]: 2 * 17 reflections even when n == 2
#define WP_FLAG_OVERFLOW 1          // more than WP_MAXSET planes of a pixel are set, or more than WP_CAND values in a centre
#define WP_FLAG_MATRIX 2            // the document's matrix or offset is not finite: nothing of it is warped
#define WP_FLAG_FOOTPRINT 0x100     // (MSAU_WARP_CPU only) a window read outside the staged footprint: a bug, the tests check for it
#define WP_LDS_INTS ((3 * WP_SRC * WP_SRC + WP_CAND * WP_THREADS) / 2 + WP_THREADS * WP_MAXSET + 4)

#define WP_Z (-0.2679491924f)       // sqrt(3) - 2
#define WP_R3 1.7320508076f
// z^k, k <= 14: the row weight at a window offset (the same for every lane)
WP_TABLE float WP_ZP[15] = {1.000000000e+00f, -2.679491924e-01f, 7.179676972e-02f, -1.923788647e-02f, 5.154776143e-03f, -1.381218105e-03f,
                            3.700962757e-04f, -9.916699820e-05f, 2.657171708e-05f, -7.119870134e-06f, 1.907763453e-06f, -5.111836765e-07f,
                            1.369712533e-07f, -3.670133671e-08f, 9.834093532e-09f};

struct WpCtx {                      // one tile of one document
    const int32_t* ids;             // the document's source planes: pixel (j, i) at j * W + i
    const int64_t* lab;
    const int64_t* aux;
    int h, w, W;                    // source extent (clipped to the canvas) and row stride
    int ho, wo, Ho, Wo;             // warped extent (clipped) and the output canvas
    double m00, m01, m10, m11, o0, o1;
    bool finite;
    int ty0, tx0;                   // the tile's first output pixel
    int y0, x0, th, tw;             // the source footprint of the tile's windows: rows y0 .. y0 + th, columns x0 .. x0 + tw
    bool any, staged;               // some pixel of the tile reads the source; the footprint is in LDS
    int n_token, n_class, Cs, dtype;
    void* grid;                     // the document's [Ho][Wo][Cs] plane of the input
    int64_t* lab_out;
    int64_t* aux_out;
    int32_t* tile_flag;
};

struct WpLds { int16_t* ids; int16_t* lab; int16_t* aux; int16_t* cand; int* set; int* flag; };
struct WpMap { const int16_t* lds; const int32_t* g32; const int64_t* g64; };

WP_DEV void wp_carve(WpLds& s, int* base) {
    int16_t* b16 = (int16_t*)base;
    s.ids = b16; s.lab = b16 + WP_SRC * WP_SRC; s.aux = b16 + 2 * WP_SRC * WP_SRC;
    s.cand = b16 + 3 * WP_SRC * WP_SRC;                             // [WP_CAND][WP_THREADS]: entry k of lane t at k * WP_THREADS + t
    s.set = base + (3 * WP_SRC * WP_SRC + WP_CAND * WP_THREADS) / 2; s.flag = s.set + WP_THREADS * WP_MAXSET;
}

// off + a * y + b * x, every operation rounded on its own, in the order of the host statement (kv_warp.source_coords)
WP_DEV double wp_coord(double o, double a, double b, double y, double x) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double t = o + a * y;
    return t + b * x;
}

WP_DEV bool wp_finite(double v) { return v - v == 0.0; }
WP_DEV int wp_value(int64_t v) { return v < 0 || v > WP_VALUE_MAX ? -1 : (int)v; }

// whole-sample mirror of a window position into [0, n-1]
WP_DEV int wp_fold(int p, int n) {
    if (n <= 1) return 0;
    for (int it = 0; it < WP_FOLD_STEPS && (p < 0 || p > n - 1); ++it) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// the interval of source positions that the windows of coordinates in [smin, smax] touch on an axis of length n; false: none in range
WP_DEV bool wp_span(double smin, double smax, int n, int& first, int& count) {
    const double lo = smin > 0.0 ? smin : 0.0, hi = smax < (double)(n - 1) ? smax : (double)(n - 1);
    if (!(lo <= hi)) return false;
    int a = (int)floor(lo) + WP_LO, b = (int)floor(hi) + WP_HI;
    if (a < 0 && -a > b) b = -a;                                    // what the mirror at 0 folds back in
    if (b > n - 1 && 2 * (n - 1) - b < a) a = 2 * (n - 1) - b;      // ... and the mirror at n - 1
    a = a < 0 ? 0 : a; b = b > n - 1 ? n - 1 : b;
    first = a; count = b - a + 1;
    return true;
}

WP_DEV void wp_ctx(WpCtx& c, int dtype, const int32_t* ids, const int64_t* lab, const int64_t* aux, const int32_t* src_sizes,
                   const double* warps, const int32_t* dst_sizes, int b, int ty, int tx, int tiles_x, int tiles, int H, int W, int Ho,
                   int Wo, int n_token, int Cs, int n_class, void* grid, int64_t* lab_out, int64_t* aux_out, int32_t* tile_flags) {
    const size_t src = (size_t)b * H * W, dst = (size_t)b * Ho * Wo;
    c.ids = ids + src; c.lab = lab + src; c.aux = aux + src;
    const int h = src_sizes[2 * b], w = src_sizes[2 * b + 1], ho = dst_sizes[2 * b], wo = dst_sizes[2 * b + 1];
    c.h = h < 0 ? 0 : (h > H ? H : h); c.w = w < 0 ? 0 : (w > W ? W : w); c.W = W;
    c.ho = ho < 0 ? 0 : (ho > Ho ? Ho : ho); c.wo = wo < 0 ? 0 : (wo > Wo ? Wo : wo); c.Ho = Ho; c.Wo = Wo;
    const double* m = warps + 6 * (size_t)b;
    c.m00 = m[0]; c.m01 = m[1]; c.m10 = m[2]; c.m11 = m[3]; c.o0 = m[4]; c.o1 = m[5];
    c.finite = wp_finite(m[0]) && wp_finite(m[1]) && wp_finite(m[2]) && wp_finite(m[3]) && wp_finite(m[4]) && wp_finite(m[5]);
    c.ty0 = ty * WP_TILE; c.tx0 = tx * WP_TILE;
    c.n_token = n_token; c.n_class = n_class; c.Cs = Cs; c.dtype = dtype;
    c.grid = (char*)grid + dst * Cs * (dtype == 0 ? 4 : 2);
    c.lab_out = lab_out + dst; c.aux_out = aux_out + dst;
    c.tile_flag = tile_flags + (size_t)b * tiles + (size_t)ty * tiles_x + tx;
    // the footprint: an affine map takes its extremes over the tile's pixels at the tile's corners (each rounded operation is monotone)
    c.any = false; c.staged = false; c.y0 = c.x0 = 0; c.th = c.tw = 0;
    const int ya = c.ty0, yb = c.ty0 + WP_TILE - 1 < c.ho - 1 ? c.ty0 + WP_TILE - 1 : c.ho - 1;
    const int xa = c.tx0, xb = c.tx0 + WP_TILE - 1 < c.wo - 1 ? c.tx0 + WP_TILE - 1 : c.wo - 1;
    if (!c.finite || c.h < 1 || c.w < 1 || yb < ya || xb < xa) return;
    double ymin = 0, ymax = 0, xmin = 0, xmax = 0;
    for (int k = 0; k < 4; ++k) {
        const double oy = (k & 1) ? yb : ya, ox = (k & 2) ? xb : xa;
        const double sy = wp_coord(c.o0, c.m00, c.m01, oy, ox), sx = wp_coord(c.o1, c.m10, c.m11, oy, ox);
        if (k == 0 || sy < ymin) ymin = sy;
        if (k == 0 || sy > ymax) ymax = sy;
        if (k == 0 || sx < xmin) xmin = sx;
        if (k == 0 || sx > xmax) xmax = sx;
    }
    if (!wp_span(ymin, ymax, c.h, c.y0, c.th) || !wp_span(xmin, xmax, c.w, c.x0, c.tw)) return;
    c.any = true;
    c.staged = c.th <= WP_SRC && c.tw <= WP_SRC;
}

// ---- phase 1: the footprint of the three canvases into LDS ----------------------------------------------------------------------------
WP_DEV void wp_ph_stage(const WpCtx& c, const WpLds& s, int tid) {
    if (tid == 0) s.flag[0] = c.finite ? 0 : WP_FLAG_MATRIX;
    if (!c.staged) return;
    const int n = c.th * c.tw;
    for (int e = tid; e < n; e += WP_THREADS) {
        const int r = e / c.tw, q = e - r * c.tw;
        const size_t at = (size_t)(c.y0 + r) * c.W + (c.x0 + q);
        s.ids[e] = (int16_t)wp_value(c.ids[at]); s.lab[e] = (int16_t)wp_value(c.lab[at]); s.aux[e] = (int16_t)wp_value(c.aux[at]);
    }
}

// ---- phase 2: one output pixel per lane -------------------------------------------------------------------------------------------------
struct WpAxis { int f; float a1, g0, g1, b2; };                     // floor(s); g at the window offsets -1, 0, 1, 2

WP_DEV void wp_taps(double s, WpAxis& a) {
    const double fl = floor(s);
    a.f = (int)fl;
    const float u = (float)(s - fl), v = 1.0f - u;
    const float b0 = v * v * v * (1.0f / 6.0f), b1 = (4.0f + u * u * (3.0f * u - 6.0f)) * (1.0f / 6.0f);
    const float b2 = (1.0f + u * (3.0f + u * (3.0f - 3.0f * u))) * (1.0f / 6.0f), b3 = u * u * u * (1.0f / 6.0f);
    const float z = WP_Z, z2 = z * z, z3 = z2 * z;                   // the taps sit at the offsets -1, 0, 1, 2: g(d) = sqrt(3) sum_t b_t z^|t - d|
    a.a1 = WP_R3 * (b0 + b1 * z + b2 * z2 + b3 * z3);
    a.g0 = WP_R3 * (b0 * z + b1 + b2 * z + b3 * z2);
    a.g1 = WP_R3 * (b0 * z2 + b1 * z + b2 + b3 * z);
    a.b2 = WP_R3 * (b0 * z3 + b1 * z2 + b2 * z + b3);
}

// g at window offset d (the same for every lane)
WP_DEV float wp_g(const WpAxis& a, int d) {
    return d <= -1 ? a.a1 * WP_ZP[-1 - d] : d == 0 ? a.g0 : d == 1 ? a.g1 : a.b2 * WP_ZP[d - 2];
}

WP_DEV int wp_rd(const WpCtx& c, const WpLds& s, const WpMap& m, int j, int i) {
    if (c.staged) {
#ifdef MSAU_WARP_CPU
        if (j < c.y0 || j >= c.y0 + c.th || i < c.x0 || i >= c.x0 + c.tw) { s.flag[0] |= WP_FLAG_FOOTPRINT; return -1; }
#endif
        return m.lds[(j - c.y0) * c.tw + (i - c.x0)];
    }
    const size_t at = (size_t)j * c.W + i;
    return wp_value(m.g32 ? (int64_t)m.g32[at] : m.g64[at]);
}

// sum of gy gx over the window offsets [lo, hi]^2 (lo <= -1, hi >= 2) at which the map holds v
WP_DEV float wp_sum(const WpCtx& c, const WpLds& s, const WpMap& m, const WpAxis& ay, const WpAxis& ax, int v, int lo, int hi) {
    float acc = 0.0f;
    for (int dy = lo; dy <= hi; ++dy) {
        const int j = wp_fold(ay.f + dy, c.h);
        float row = 0.0f, g = ax.a1;
        for (int dx = -1; dx >= lo; --dx) {
            if (wp_rd(c, s, m, j, wp_fold(ax.f + dx, c.w)) == v) row += g;
            g *= WP_Z;
        }
        if (wp_rd(c, s, m, j, wp_fold(ax.f, c.w)) == v) row += ax.g0;
        if (wp_rd(c, s, m, j, wp_fold(ax.f + 1, c.w)) == v) row += ax.g1;
        g = ax.b2;
        for (int dx = 2; dx <= hi; ++dx) {
            if (wp_rd(c, s, m, j, wp_fold(ax.f + dx, c.w)) == v) row += g;
            g *= WP_Z;
        }
        acc += wp_g(ay, dy) * row;
    }
    return acc;
}

// the values in [first, limit) whose plane is set at the lane's pixel, left at the front of the lane's list -> their number
WP_DEV int wp_set_values(const WpCtx& c, const WpLds& s, const WpMap& m, const WpAxis& ay, const WpAxis& ax, int tid, int first, int limit) {
    int16_t* list = s.cand + tid;
    int n = 0;
    for (int dy = WP_CLO; dy <= WP_CHI; ++dy) {                      // the distinct values of the centre
        const int j = wp_fold(ay.f + dy, c.h);
        int prev = -1;
        for (int dx = WP_CLO; dx <= WP_CHI; ++dx) {
            const int v = wp_rd(c, s, m, j, wp_fold(ax.f + dx, c.w));
            if (v == prev) continue;
            prev = v;
            if (v < first || v >= limit) continue;
            bool seen = false;
            for (int k = 0; k < n; ++k) seen = seen || list[k * WP_THREADS] == v;
            if (seen) continue;
            if (n < WP_CAND) list[n++ * WP_THREADS] = (int16_t)v;
            else s.flag[0] = s.flag[0] | WP_FLAG_OVERFLOW;            // (lanes race to store the same bit: LDS, no atomic needed)
        }
    }
    int kept = 0;
    for (int k = 0; k < n; ++k) {                                    // ... whose centre sum can carry a set plane
        const int v = list[k * WP_THREADS];
        if (wp_sum(c, s, m, ay, ax, v, WP_CLO, WP_CHI) > WP_CENTRE_MIN) list[kept++ * WP_THREADS] = (int16_t)v;
    }
    int set = 0;
    for (int k = 0; k < kept; ++k) {                                 // ... whose plane is set
        const int v = list[k * WP_THREADS];
        if (255.0f * wp_sum(c, s, m, ay, ax, v, WP_LO, WP_HI) > 64.5f) list[set++ * WP_THREADS] = (int16_t)v;
    }
    return set;
}

// the label of a target map: 1 if plane 1 is set, else the smallest set plane >= 2, else 0 (plane 0 plays no part)
WP_DEV int wp_label_of(const WpCtx& c, const WpLds& s, const WpMap& m, const WpAxis& ay, const WpAxis& ax, int tid) {
    const int n = wp_set_values(c, s, m, ay, ax, tid, 1, c.n_class);
    int best = 0x7fffffff;
    for (int k = 0; k < n; ++k) {
        const int v = s.cand[k * WP_THREADS + tid];
        if (v == 1) return 1;
        best = v < best ? v : best;
    }
    return best != 0x7fffffff ? best : 0;
}

WP_DEV void wp_ph_pixel(const WpCtx& c, const WpLds& s, int tid) {
    const int oy = c.ty0 + tid / WP_TILE, ox = c.tx0 + tid % WP_TILE;
    int set[WP_MAXSET] = {-1, -1, -1, -1};
    int64_t lab = -1, aux = -1;
    if (oy < c.ho && ox < c.wo) {
        lab = 0; aux = 0;
        const double sy = wp_coord(c.o0, c.m00, c.m01, (double)oy, (double)ox), sx = wp_coord(c.o1, c.m10, c.m11, (double)oy, (double)ox);
        const bool in = c.any && sy >= 0.0 && sy <= (double)(c.h - 1) && sx >= 0.0 && sx <= (double)(c.w - 1);
        if (in) {
            WpAxis ay, ax;
            wp_taps(sy, ay);
            wp_taps(sx, ax);
            const WpMap mi = {s.ids, c.ids, 0}, ml = {s.lab, 0, c.lab}, ma = {s.aux, 0, c.aux};
            const int n = wp_set_values(c, s, mi, ay, ax, tid, 0, c.n_token);
            if (n > WP_MAXSET) s.flag[0] = s.flag[0] | WP_FLAG_OVERFLOW;
#pragma unroll
            for (int k = 0; k < WP_MAXSET; ++k) set[k] = k < n ? s.cand[k * WP_THREADS + tid] : -1;
            lab = wp_label_of(c, s, ml, ay, ax, tid);
            aux = wp_label_of(c, s, ma, ay, ax, tid);
        }
    }
    int* mine = s.set + tid * WP_MAXSET;
#pragma unroll
    for (int k = 0; k < WP_MAXSET; ++k) mine[k] = set[k];
    if (oy < c.Ho && ox < c.Wo) {
        const size_t at = (size_t)oy * c.Wo + ox;
        c.lab_out[at] = lab; c.aux_out[at] = aux;
    }
}

// ---- phase 3: the tile's channels, 8 per lane and store ----------------------------------------------------------------------------------
WP_DEV void wp_ph_store(const WpCtx& c, const WpLds& s, int tid) {
    if (tid == 0) *c.tile_flag = s.flag[0];
    const int groups = c.Cs >> 3, n = WP_THREADS * groups;
    for (int e = tid; e < n; e += WP_THREADS) {
        const int pix = e / groups, g = e - pix * groups;
        const int oy = c.ty0 + pix / WP_TILE, ox = c.tx0 + pix % WP_TILE;
        if (oy >= c.Ho || ox >= c.Wo) continue;
        const int* set = s.set + pix * WP_MAXSET;
        const int s0 = set[0], s1 = set[1], s2 = set[2], s3 = set[3];
        bool on[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int ch = g * 8 + k;
            on[k] = ch == s0 || ch == s1 || ch == s2 || ch == s3;
        }
        const size_t at = ((size_t)oy * c.Wo + ox) * c.Cs + (size_t)g * 8;
        if (c.dtype == 0) {
            float* out = (float*)c.grid + at;
#ifdef MSAU_WARP_CPU
            for (int k = 0; k < 8; ++k) out[k] = on[k] ? 1.0f : 0.0f;
#else
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            const f32x4 a = {on[0] ? 1.0f : 0.0f, on[1] ? 1.0f : 0.0f, on[2] ? 1.0f : 0.0f, on[3] ? 1.0f : 0.0f};
            const f32x4 b = {on[4] ? 1.0f : 0.0f, on[5] ? 1.0f : 0.0f, on[6] ? 1.0f : 0.0f, on[7] ? 1.0f : 0.0f};
            *reinterpret_cast<f32x4*>(out) = a;
            *reinterpret_cast<f32x4*>(out + 4) = b;
#endif
        } else {
            uint16_t* out = (uint16_t*)c.grid + at;                         // bf16: 1.0 is 0x3f80
#ifdef MSAU_WARP_CPU
            for (int k = 0; k < 8; ++k) out[k] = on[k] ? 0x3f80 : 0;
#else
            typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
            u16x8 v;
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = on[k] ? (unsigned short)0x3f80 : (unsigned short)0;
            *reinterpret_cast<u16x8*>(out) = v;
#endif
        }
    }
}

WP_DEV void wp_body(const WpCtx& c, const WpLds& s) {
    WP_PHASE(wp_ph_stage);
    WP_PHASE(wp_ph_pixel);
    WP_PHASE(wp_ph_store);
}

// ---- the elastic warp: msau_kv_elastic_train ---------------------------------------------------------------------------------------------
// The generator's elastic_transform (utils/image_util.py:58-90; kv_warp.py "the elastic warp"): output pixel (oy, ox)
// of every one-hot plane x 255 is scipy's map_coordinates(order=1, mode "constant") at
//   sy = oy + fy[oy, ox] * alpha_y,  sx = ox + fx[oy, ox] * alpha_x     (float64, the product rounded, then the sum; fields uint8)
// 0 outside [0, h-1] x [0, w-1], else with uy = sy - floor(sy), ux = sx - floor(sx), p = 255 [canvas(tap) == c]
//   grey = (1 - uy) * ((1 - ux) * p00 + ux * p01) + uy * ((1 - ux) * p10 + ux * p11)       (this order, nothing fused)
// on the taps floor(s) and floor(s) + 1, the latter clamped to n - 1 where its weight is 0; the plane is set iff grey >= 64.5 (scipy
// stores grey + 0.5 truncated, the generator keeps > 64).  The four weights sum to 1 and a set plane needs 0.2529 of them, so at most
// three planes of a pixel are set: the WP_MAXSET slots always suffice.  The output has the source's extent.
//
// Same tiles, same outputs and same rules as above (every element written once by one lane, no atomics, a word per tile folded by the
// flags kernel) with another phase 2: a lane reads its pixel's two field bytes and the 4 taps of each canvas straight from global
// memory -- neighbouring lanes read neighbouring addresses, and 12 reads per pixel earn no staging -- and evaluates the grey level of
// each of the at most 4 distinct tap values in float64, exactly as the host statement does: the outputs equal it to the bit.  No LDS
// beyond the set slots that phase 3 (wp_ph_store, unchanged) reads.  An alpha that is not finite flags the document
// (WP_FLAG_MATRIX) and nothing of it is resampled; a negative one is legal, its coordinates simply fall outside.
#define WE_LDS_INTS (WP_THREADS * WP_MAXSET + 4)

struct WeCtx {
    WpCtx c;                        // what phase 3 reads, and the source planes and extents (ho == h, wo == w, clipped to the canvases)
    const uint8_t* fld;             // the document's [H][W][2] = (fy, fx)
    double alpha_y, alpha_x;
};

struct WeTaps { double vy, uy, vx, ux; size_t at[4]; };             // weights of floor / floor + 1 per axis; addresses of p00, p01, p10, p11

// A product that is to be rounded before it is added to.  The library is built with -ffp-contract=fast, under which the backend
// fuses a multiplication into the addition it feeds wherever it still sees it, whatever the pragma says; an empty asm statement
// that takes the product in and out of its register hides it (no instruction is emitted).  The plain C++ form is built with
// -ffp-contract=off.
WP_DEV double we_rounded(double v) {
#ifndef MSAU_WARP_CPU
    asm("" : "+v"(v));
#endif
    return v;
}

// o + f * alpha, the product rounded, then the sum (kv_warp.elastic_coords)
WP_DEV double we_coord(double o, double f, double alpha) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double d = we_rounded(f * alpha);
    return o + d;
}

WP_DEV void we_axis(double s, int n, int& q0, int& q1, double& v, double& u) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double fl = floor(s);
    q0 = (int)fl;
    q1 = q0 + 1 < n ? q0 + 1 : n - 1;
    u = s - fl;
    v = 1.0 - u;
}

// the grey level of plane [canvas == v] from the four tap values, in the statement's order
WP_DEV double we_grey(const WeTaps& t, const int* tap, int v) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double p00 = tap[0] == v ? 255.0 : 0.0, p01 = tap[1] == v ? 255.0 : 0.0;
    const double p10 = tap[2] == v ? 255.0 : 0.0, p11 = tap[3] == v ? 255.0 : 0.0;
    const double a0 = we_rounded(t.vx * p00), a1 = we_rounded(t.ux * p01), b0 = we_rounded(t.vx * p10), b1 = we_rounded(t.ux * p11);
    const double top = a0 + a1, bot = b0 + b1;
    const double y0 = we_rounded(t.vy * top), y1 = we_rounded(t.uy * bot);
    return y0 + y1;
}

// the distinct tap values in [first, limit) whose plane is set -> out[0 .. n), n <= 4 (by the weights, n <= 3)
WP_DEV int we_set_values(const WeTaps& t, const int* tap, int first, int limit, int* out) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int v = tap[k];
        bool seen = v < first || v >= limit;
#pragma unroll
        for (int q = 0; q < k; ++q) seen = seen || tap[q] == v;
        if (seen) continue;
        if (we_grey(t, tap, v) >= 64.5) out[n++] = v;
    }
    return n;
}

WP_DEV int we_label_of(const WeTaps& t, const int* tap, int n_class) {
    int got[4];
    const int n = we_set_values(t, tap, 1, n_class, got);
    int best = 0x7fffffff;
    for (int k = 0; k < n; ++k) {
        if (got[k] == 1) return 1;
        best = got[k] < best ? got[k] : best;
    }
    return best != 0x7fffffff ? best : 0;
}

WP_DEV void we_ctx(WeCtx& e, int dtype, const int32_t* ids, const int64_t* lab, const int64_t* aux, const int32_t* src_sizes,
                   const uint8_t* fields, const double* alphas, int b, int ty, int tx, int tiles_x, int tiles, int H, int W, int Ho,
                   int Wo, int n_token, int Cs, int n_class, void* grid, int64_t* lab_out, int64_t* aux_out, int32_t* tile_flags) {
    WpCtx& c = e.c;
    const size_t src = (size_t)b * H * W, dst = (size_t)b * Ho * Wo;
    c.ids = ids + src; c.lab = lab + src; c.aux = aux + src;
    e.fld = fields + 2 * src;
    const int h = src_sizes[2 * b], w = src_sizes[2 * b + 1];
    c.h = h < 0 ? 0 : (h > H ? H : h); c.w = w < 0 ? 0 : (w > W ? W : w); c.W = W;
    c.ho = c.h > Ho ? Ho : c.h; c.wo = c.w > Wo ? Wo : c.w; c.Ho = Ho; c.Wo = Wo;
    e.alpha_y = alphas[2 * (size_t)b]; e.alpha_x = alphas[2 * (size_t)b + 1];
    c.m00 = c.m11 = 1.0; c.m01 = c.m10 = c.o0 = c.o1 = 0.0;
    c.finite = wp_finite(e.alpha_y) && wp_finite(e.alpha_x);
    c.ty0 = ty * WP_TILE; c.tx0 = tx * WP_TILE;
    c.y0 = c.x0 = 0; c.th = c.tw = 0; c.any = c.h >= 1 && c.w >= 1; c.staged = false;
    c.n_token = n_token; c.n_class = n_class; c.Cs = Cs; c.dtype = dtype;
    c.grid = (char*)grid + dst * Cs * (dtype == 0 ? 4 : 2);
    c.lab_out = lab_out + dst; c.aux_out = aux_out + dst;
    c.tile_flag = tile_flags + (size_t)b * tiles + (size_t)ty * tiles_x + tx;
}

// ---- phase 2 of the elastic warp: one output pixel per lane, taps from global memory ---------------------------------------------------
WP_DEV void we_ph_pixel(const WeCtx& e, const WpLds& s, int tid) {
    const WpCtx& c = e.c;
    if (tid == 0) s.flag[0] = c.finite ? 0 : WP_FLAG_MATRIX;         // (the only store to the flag: a pixel cannot overflow its slots)
    const int oy = c.ty0 + tid / WP_TILE, ox = c.tx0 + tid % WP_TILE;
    int set[WP_MAXSET] = {-1, -1, -1, -1};
    int64_t lab = -1, aux = -1;
    if (oy < c.ho && ox < c.wo) {                                     // inside the document: oy < h <= H, ox < w <= W
        lab = 0; aux = 0;
        if (c.finite) {
            const uint8_t* f = e.fld + ((size_t)oy * c.W + ox) * 2;
            const double sy = we_coord((double)oy, (double)f[0], e.alpha_y), sx = we_coord((double)ox, (double)f[1], e.alpha_x);
            if (sy >= 0.0 && sy <= (double)(c.h - 1) && sx >= 0.0 && sx <= (double)(c.w - 1)) {
                WeTaps t;
                int j0, j1, i0, i1;
                we_axis(sy, c.h, j0, j1, t.vy, t.uy);                 // 0 <= j0 <= j1 <= h - 1
                we_axis(sx, c.w, i0, i1, t.vx, t.ux);
                t.at[0] = (size_t)j0 * c.W + i0; t.at[1] = (size_t)j0 * c.W + i1;
                t.at[2] = (size_t)j1 * c.W + i0; t.at[3] = (size_t)j1 * c.W + i1;
                int tap[4], got[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) tap[k] = wp_value(c.ids[t.at[k]]);
                const int n = we_set_values(t, tap, 0, c.n_token, got);
#pragma unroll
                for (int k = 0; k < WP_MAXSET; ++k) set[k] = k < n ? got[k] : -1;
#pragma unroll
                for (int k = 0; k < 4; ++k) tap[k] = wp_value(c.lab[t.at[k]]);
                lab = we_label_of(t, tap, c.n_class);
#pragma unroll
                for (int k = 0; k < 4; ++k) tap[k] = wp_value(c.aux[t.at[k]]);
                aux = we_label_of(t, tap, c.n_class);
            }
        }
    }
    int* mine = s.set + tid * WP_MAXSET;
#pragma unroll
    for (int k = 0; k < WP_MAXSET; ++k) mine[k] = set[k];
    if (oy < c.Ho && ox < c.Wo) {
        const size_t at = (size_t)oy * c.Wo + ox;
        c.lab_out[at] = lab; c.aux_out[at] = aux;
    }
}

WP_DEV void we_carve(WpLds& s, int* base) {
    s.ids = s.lab = s.aux = s.cand = 0;                             // nothing is staged and no lane keeps a list
    s.set = base; s.flag = base + WP_THREADS * WP_MAXSET;
}

WP_DEV void we_body(const WeCtx& e, const WpLds& s) {
    { const WeCtx& c = e; WP_PHASE(we_ph_pixel); }
    { const WpCtx& c = e.c; WP_PHASE(wp_ph_store); }
}

#ifdef MSAU_WARP_CPU
extern "C" int64_t msau_kv_elastic_train_ws_ints(int B, int Ho, int Wo) {
    return (int64_t)B * ((Ho + WP_TILE - 1) / WP_TILE) * ((Wo + WP_TILE - 1) / WP_TILE);
}

// the launch, lane by lane on the host: same arguments as msau_kv_elastic_train without the stream
extern "C" int msau_kv_elastic_train_cpu(int dtype, const int32_t* ids, const int64_t* labels, const int64_t* aux_labels,
                                         const int32_t* src_sizes, const uint8_t* fields, const double* alphas, int B, int H, int W, int Ho,
                                         int Wo, int n_token, int Cs, int n_class, void* grid, int64_t* labels_out, int64_t* aux_out,
                                         int32_t* flags, int32_t* ws) {
    if (n_token > WP_VALUE_MAX + 1 || n_class > WP_VALUE_MAX + 1) return 2;
    int lds[WE_LDS_INTS];
    const int tiles_y = (Ho + WP_TILE - 1) / WP_TILE, tiles_x = (Wo + WP_TILE - 1) / WP_TILE, tiles = tiles_x * tiles_y;
    for (int b = 0; b < B; ++b) {
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx) {
                WeCtx e;
                we_ctx(e, dtype, ids, labels, aux_labels, src_sizes, fields, alphas, b, ty, tx, tiles_x, tiles, H, W, Ho, Wo, n_token,
                       Cs, n_class, grid, labels_out, aux_out, ws);
                WpLds s;
                we_carve(s, lds);
                we_body(e, s);
            }
        int f = 0;
        for (int t = 0; t < tiles; ++t) f |= ws[(size_t)b * tiles + t];
        flags[b] = f;
    }
    return 0;
}

extern "C" int64_t msau_kv_warp_train_ws_ints(int B, int Ho, int Wo) {
    return (int64_t)B * ((Ho + WP_TILE - 1) / WP_TILE) * ((Wo + WP_TILE - 1) / WP_TILE);
}

// the launch, lane by lane on the host: same arguments as msau_kv_warp_train without the stream
extern "C" int msau_kv_warp_train_cpu(int dtype, const int32_t* ids, const int64_t* labels, const int64_t* aux_labels,
                                      const int32_t* src_sizes, const double* warps, const int32_t* dst_sizes, int B, int H, int W, int Ho,
                                      int Wo, int n_token, int Cs, int n_class, void* grid, int64_t* labels_out, int64_t* aux_out,
                                      int32_t* flags, int32_t* ws) {
    if (n_token > WP_VALUE_MAX + 1 || n_class > WP_VALUE_MAX + 1) return 2;
    int* lds = (int*)malloc(sizeof(int) * WP_LDS_INTS);
    if (!lds) return 1;
    const int tiles_y = (Ho + WP_TILE - 1) / WP_TILE, tiles_x = (Wo + WP_TILE - 1) / WP_TILE, tiles = tiles_x * tiles_y;
    for (int b = 0; b < B; ++b) {
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx) {
                WpCtx c;
                wp_ctx(c, dtype, ids, labels, aux_labels, src_sizes, warps, dst_sizes, b, ty, tx, tiles_x, tiles, H, W, Ho, Wo, n_token,
                       Cs, n_class, grid, labels_out, aux_out, ws);
                WpLds s;
                wp_carve(s, lds);
                wp_body(c, s);
            }
        int f = 0;
        for (int t = 0; t < tiles; ++t) f |= ws[(size_t)b * tiles + t];
        flags[b] = f;
    }
    free(lds);
    return 0;
}
#else

__global__ void __launch_bounds__(WP_THREADS)
kv_warp_train_kernel(int dtype, const int32_t* ids, const int64_t* labels, const int64_t* aux_labels, const int32_t* src_sizes,
                     const double* warps, const int32_t* dst_sizes, int H, int W, int Ho, int Wo, int n_token, int Cs, int n_class,
                     void* grid, int64_t* labels_out, int64_t* aux_out, int32_t* ws) {
    __shared__ int wp_lds[WP_LDS_INTS];
    WpCtx c;
    wp_ctx(c, dtype, ids, labels, aux_labels, src_sizes, warps, dst_sizes, (int)blockIdx.z, (int)blockIdx.y, (int)blockIdx.x,
           (int)gridDim.x, (int)(gridDim.x * gridDim.y), H, W, Ho, Wo, n_token, Cs, n_class, grid, labels_out, aux_out, ws);
    WpLds s;
    wp_carve(s, wp_lds);
    wp_body(c, s);
}

// flags[b] = the tiles' words of document b, or-ed: one wavefront per document, every lane a strided share, lane 0 stores
__global__ void __launch_bounds__(64)
kv_warp_flags_kernel(const int32_t* ws, int tiles, int32_t* flags) {
    __shared__ int part[64];
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    int f = 0;
    for (int t = lane; t < tiles; t += 64) f |= ws[(size_t)b * tiles + t];
    part[lane] = f;
    __syncthreads();
    if (lane == 0) {
        for (int k = 1; k < 64; ++k) f |= part[k];
        flags[b] = f;
    }
}

extern "C" int64_t msau_kv_warp_train_ws_ints(int B, int Ho, int Wo) {
    if (B <= 0 || Ho <= 0 || Wo <= 0) return 0;
    return (int64_t)B * cdiv(Ho, WP_TILE) * cdiv(Wo, WP_TILE);
}

extern "C" int msau_kv_warp_train(void* stream, int dtype, const int32_t* ids, const int64_t* labels, const int64_t* aux_labels,
                                  const int32_t* src_sizes, const double* warps, const int32_t* dst_sizes, int B, int H, int W, int Ho,
                                  int Wo, int n_token, int Cs, int n_class, void* grid, int64_t* labels_out, int64_t* aux_out,
                                  int32_t* flags, int32_t* ws) {
    MSAU_CHECK_ARG(ids && labels && aux_labels && src_sizes && warps && dst_sizes && grid && labels_out && aux_out && flags && ws,
                   "kv_warp_train: null pointer");
    MSAU_CHECK_ARG(dtype == 0 || dtype == 1, "kv_warp_train: dtype %d is neither MSAU_F32 nor MSAU_BF16", dtype);
    MSAU_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && (int64_t)B * H * W < (1ll << 31)
                   && (int64_t)B * Ho * Wo < (1ll << 31), "kv_warp_train: bad shape B = %d, H = %d, W = %d, Ho = %d, Wo = %d", B, H, W, Ho, Wo);
    MSAU_CHECK_ARG(cdiv(Ho, WP_TILE) <= 65535, "kv_warp_train: Ho = %d is more than 65535 tiles", Ho);
    MSAU_CHECK_ARG(n_token > 0 && n_class > 0 && Cs > 0 && Cs % 8 == 0 && n_token <= Cs && n_token <= WP_VALUE_MAX + 1
                   && n_class <= WP_VALUE_MAX + 1,
                   "kv_warp_train: n_token = %d, Cs = %d, n_class = %d (need n_token <= Cs, Cs %% 8 == 0, both counts <= 32767)", n_token,
                   Cs, n_class);
    MSAU_CHECK_ARG((uintptr_t)grid % 16 == 0 && ((uintptr_t)labels | (uintptr_t)aux_labels | (uintptr_t)labels_out | (uintptr_t)aux_out
                                                 | (uintptr_t)warps) % 8 == 0
                   && ((uintptr_t)ids | (uintptr_t)src_sizes | (uintptr_t)dst_sizes | (uintptr_t)flags | (uintptr_t)ws) % 4 == 0,
                   "kv_warp_train: the input must be 16-byte aligned, every other array to its element size");
    static_assert(WP_TILE * WP_TILE == WP_THREADS, "kv_warp_train: a lane per pixel of the tile");
    static_assert(sizeof(int) * WP_LDS_INTS <= 64 * 1024, "kv_warp_train: the LDS of a workgroup");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tiles_x = cdiv(Wo, WP_TILE), tiles_y = cdiv(Ho, WP_TILE);
    hipLaunchKernelGGL(kv_warp_train_kernel, dim3(tiles_x, tiles_y, B), dim3(WP_THREADS), 0, st, dtype, ids, labels, aux_labels,
                       src_sizes, warps, dst_sizes, H, W, Ho, Wo, n_token, Cs, n_class, grid, labels_out, aux_out, ws);
    MSAU_CHECK_LAUNCH("kv_warp_train");
    hipLaunchKernelGGL(kv_warp_flags_kernel, dim3(B), dim3(64), 0, st, ws, tiles_x * tiles_y, flags);
    MSAU_CHECK_LAUNCH("kv_warp_flags");
    return 0;
}

__global__ void __launch_bounds__(WP_THREADS)
kv_elastic_train_kernel(int dtype, const int32_t* ids, const int64_t* labels, const int64_t* aux_labels, const int32_t* src_sizes,
                        const uint8_t* fields, const double* alphas, int H, int W, int Ho, int Wo, int n_token, int Cs, int n_class,
                        void* grid, int64_t* labels_out, int64_t* aux_out, int32_t* ws) {
    __shared__ int we_lds[WE_LDS_INTS];
    WeCtx e;
    we_ctx(e, dtype, ids, labels, aux_labels, src_sizes, fields, alphas, (int)blockIdx.z, (int)blockIdx.y, (int)blockIdx.x,
           (int)gridDim.x, (int)(gridDim.x * gridDim.y), H, W, Ho, Wo, n_token, Cs, n_class, grid, labels_out, aux_out, ws);
    WpLds s;
    we_carve(s, we_lds);
    we_body(e, s);
}

extern "C" int64_t msau_kv_elastic_train_ws_ints(int B, int Ho, int Wo) { return msau_kv_warp_train_ws_ints(B, Ho, Wo); }

extern "C" int msau_kv_elastic_train(void* stream, int dtype, const int32_t* ids, const int64_t* labels, const int64_t* aux_labels,
                                     const int32_t* src_sizes, const uint8_t* fields, const double* alphas, int B, int H, int W, int Ho,
                                     int Wo, int n_token, int Cs, int n_class, void* grid, int64_t* labels_out, int64_t* aux_out,
                                     int32_t* flags, int32_t* ws) {
    MSAU_CHECK_ARG(ids && labels && aux_labels && src_sizes && fields && alphas && grid && labels_out && aux_out && flags && ws,
                   "kv_elastic_train: null pointer");
    MSAU_CHECK_ARG(dtype == 0 || dtype == 1, "kv_elastic_train: dtype %d is neither MSAU_F32 nor MSAU_BF16", dtype);
    MSAU_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && (int64_t)B * H * W < (1ll << 31)
                   && (int64_t)B * Ho * Wo < (1ll << 31), "kv_elastic_train: bad shape B = %d, H = %d, W = %d, Ho = %d, Wo = %d", B, H, W, Ho,
                   Wo);
    MSAU_CHECK_ARG(cdiv(Ho, WP_TILE) <= 65535, "kv_elastic_train: Ho = %d is more than 65535 tiles", Ho);
    MSAU_CHECK_ARG(n_token > 0 && n_class > 0 && Cs > 0 && Cs % 8 == 0 && n_token <= Cs && n_token <= WP_VALUE_MAX + 1
                   && n_class <= WP_VALUE_MAX + 1,
                   "kv_elastic_train: n_token = %d, Cs = %d, n_class = %d (need n_token <= Cs, Cs %% 8 == 0, both counts <= 32767)", n_token,
                   Cs, n_class);
    MSAU_CHECK_ARG((uintptr_t)grid % 16 == 0 && ((uintptr_t)labels | (uintptr_t)aux_labels | (uintptr_t)labels_out | (uintptr_t)aux_out
                                                 | (uintptr_t)alphas) % 8 == 0
                   && ((uintptr_t)ids | (uintptr_t)src_sizes | (uintptr_t)flags | (uintptr_t)ws) % 4 == 0,
                   "kv_elastic_train: the input must be 16-byte aligned, every other array to its element size");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tiles_x = cdiv(Wo, WP_TILE), tiles_y = cdiv(Ho, WP_TILE);
    hipLaunchKernelGGL(kv_elastic_train_kernel, dim3(tiles_x, tiles_y, B), dim3(WP_THREADS), 0, st, dtype, ids, labels, aux_labels,
                       src_sizes, fields, alphas, H, W, Ho, Wo, n_token, Cs, n_class, grid, labels_out, aux_out, ws);
    MSAU_CHECK_LAUNCH("kv_elastic_train");
    hipLaunchKernelGGL(kv_warp_flags_kernel, dim3(B), dim3(64), 0, st, ws, tiles_x * tiles_y, flags);
    MSAU_CHECK_LAUNCH("kv_warp_flags");
    return 0;
}
#endif
