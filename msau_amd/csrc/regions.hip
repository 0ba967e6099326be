// Region extraction for key-value inference (inference/kv_model.py `_extract_value`, the per-pixel part): from the uint8 class
// map the head writes, per document and per field class c >= 2
//   M_c   = closing of (argmax == c) with a 1 x 3 element, zero outside the DOCUMENT (morph_util.r_closing(mask, (1, 3)))
//   comps = the 4-connected components of M_c, numbered by the raster position of their first pixel (scipy.ndimage.label),
//           each with its first pixel, its half-open bounding box (find_objects) and its pixel count
//   pairs = for (component k, text line v >= 1): n_under = pixels of k whose line id is v; cp_min / cp_max = smallest / largest
//           non-zero character position over the pixels of k inside line v's box
// One workgroup per (document, class); the whole document lives in LDS:
//   labels   int32 [RG_MAXPIX]      union-find forest, parent <= child, so a root is its component's smallest linear index
//                                   (the large form, for documents of more pixels: h * w int32 of a workspace in device memory,
//                                   indexed alike; everything else as here)
//   pairs    4 x uint32 [RG_HASH]   open-addressing hash keyed (k << 16) | v, sorted in place (bitonic) before it is written
//   comps    6 x int32 [RG_MAXK]    first pixel, box, count
// The scored form (rg_body<true>) adds, per component, the sum over its pixels of q(p) = rint(p * 65536), p the probability of the
// workgroup's class at the pixel (fp32 [B][H][W][n_class] on the canvas): 64-bit integers in two of the component tables, which
// are dead once rg_ph_write has run, written to scores[roff + k] beside the region record of the same row.
// Every loop is a counted loop whose bound follows from the document's pixel count (or from the sizes of the LDS tables); a
// document that does not fit, a table that is full and a labelling that has not converged set the document's overflow flag
// and end the workgroup.  The results are integers and do not depend on arrival order: the component numbers are ranks of root
// indices, the pair list is sorted by key; only the position of a class's slice inside its document's lists (header) depends on
// which workgroup reserved first.
//
// The body is written as phases between workgroup barriers; with -DMSAU_REGIONS_CPU the same phases compile as plain C++ and
// the lanes of a phase run one after another (tests/test_regions_cpu.py builds that form with the host compiler).
#ifdef MSAU_REGIONS_CPU
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#define RG_DEV static inline
#define RG_PHASE(fn, ...) do { for (int t__ = 0; t__ < RG_THREADS; ++t__) fn(c, s, t__, ##__VA_ARGS__); } while (0)
RG_DEV int rg_amin(int* p, int v) { int o = *p; if (v < o) *p = v; return o; }
RG_DEV int rg_amax(int* p, int v) { int o = *p; if (v > o) *p = v; return o; }
RG_DEV int rg_aadd(int* p, int v) { int o = *p; *p = o + v; return o; }
RG_DEV void rg_aadd64(long long* p, long long v) { *p += v; }
RG_DEV int rg_aor(int* p, int v) { int o = *p; *p = o | v; return o; }
RG_DEV unsigned rg_acas(unsigned* p, unsigned cmp, unsigned v) { unsigned o = *p; if (o == cmp) *p = v; return o; }
RG_DEV int rg_ld(const int* p) { return *p; }
RG_DEV int rg_rint(float v) { return (int)lrintf(v); }                    // to nearest even (the default rounding mode)
#define RG_SYNC() do { } while (0)
#else
#include "msau_common.h"
#define RG_DEV __device__ __forceinline__
#define RG_PHASE(fn, ...) do { fn(c, s, (int)threadIdx.x, ##__VA_ARGS__); __syncthreads(); } while (0)
RG_DEV int rg_amin(int* p, int v) { return atomicMin(p, v); }
RG_DEV int rg_amax(int* p, int v) { return atomicMax(p, v); }
RG_DEV int rg_aadd(int* p, int v) { return atomicAdd(p, v); }
RG_DEV void rg_aadd64(long long* p, long long v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }
RG_DEV int rg_aor(int* p, int v) { return atomicOr(p, v); }
RG_DEV unsigned rg_acas(unsigned* p, unsigned cmp, unsigned v) { return atomicCAS(p, cmp, v); }
// a label another wave may change in the same phase: never from a register or (large form) from the L1, always a value written
RG_DEV int rg_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
RG_DEV int rg_rint(float v) { return __float2int_rn(v); }                 // to nearest even
#define RG_SYNC() __syncthreads()
#endif
// a uniform exit: every lane reads the flags, THEN a barrier, so that no lane of the next phase can change them under a reader
#define RG_CHECK() do { const int f__ = s.misc[RG_FAIL]; RG_SYNC(); if (f__) return f__; } while (0)

#define RG_THREADS 1024
#define RG_MAXPIX 24576
#define RG_MAXK 1024
#define RG_HASH 2048
#define RG_REGION_INTS 8
#define RG_PAIR_INTS 4
#define RG_MAXLINES 65535
#define RG_LARGE_MAXPIX (0x7FFFFFFF - 2 * RG_THREADS)   // the large form: p + RG_THREADS and lane * chunk + i stay in an int
#define RG_LARGE_DOCS 32                                // documents per launch of the large form (their list is a kernel argument)
#define RG_EMPTY 0xFFFFFFFFu
#define RG_BG (-1)
enum { RG_OVF_PIXELS = 1, RG_OVF_LABEL = 2, RG_OVF_REGIONS = 4, RG_OVF_PAIRS = 8, RG_OVF_LINES = 16 };
enum { RG_FAIL = 0, RG_NCOMP = 1, RG_NPAIR = 2, RG_ROFF = 3, RG_POFF = 4, RG_MISC = 8 };

struct RgCtx {                      // one (document, class)
    const uint8_t* cls;             // the document's planes on the canvas: pixel (y, x) at y * W + x
    const uint16_t* line;
    const uint16_t* chr;
    const int32_t* boxes;           // the document's lines [n_lines][4] = (x1, y1, x2, y2)
    int n_lines, h, w, W, c;
    int32_t* hdr;                   // the document's header [n_class][4]; row 0 holds the two cursors
    int32_t* regions;               // the document's slices of the output lists
    int32_t* pairs;
    int cap_regions, cap_pairs;
    const float* probs;             // the scored form only: the document's probabilities, pixel (y, x) class k at (y * W + x) * n_class + k
    int64_t* scores;                //                       the document's rows [cap_regions], beside `regions`
    int n_class;
};

struct RgLds {
    int* L;                                          // [RG_MAXPIX] in LDS, or [h * w] of the workspace (large form)
    unsigned* hk; int* hn; int* hmn; int* hmx;       // [RG_HASH]
    int* cfirst; int* cy0; int* cy1; int* cx0; int* cx1; int* ccnt;   // [RG_MAXK]
    long long* sum;                                  // [RG_MAXK] over cy0 and cy1, once rg_ph_write has read them (scored form)
    int* scan;                                       // [RG_THREADS]
    int* part;                                       // [32]
    int* misc;                                       // [RG_MISC]
};
#define RG_TABLE_INTS (4 * RG_HASH + 6 * RG_MAXK + RG_THREADS + 32 + RG_MISC)
#define RG_LDS_INTS (RG_MAXPIX + RG_TABLE_INTS)

// L: the labels; base: RG_TABLE_INTS for the tables
RG_DEV void rg_carve(RgLds& s, int* L, int* base) {
    s.L = L;
    s.hk = (unsigned*)base; base += RG_HASH;
    s.hn = base; base += RG_HASH;
    s.hmn = base; base += RG_HASH;
    s.hmx = base; base += RG_HASH;
    s.cfirst = base; base += RG_MAXK;
    s.cy0 = base; s.sum = (long long*)base; base += RG_MAXK;
    s.cy1 = base; base += RG_MAXK;
    s.cx0 = base; base += RG_MAXK;
    s.cx1 = base; base += RG_MAXK;
    s.ccnt = base; base += RG_MAXK;
    s.scan = base; base += RG_THREADS;
    s.part = base; base += 32;
    s.misc = base;
}

// closing with a 1 x 3 element, zero outside [0, w): D(x) = m(x-1) | m(x) | m(x+1), M(x) = D(x-1) & D(x) & D(x+1) with D = 0
// outside, so M(0) = M(w-1) = 0 and M(x) reads m(x-2 .. x+2)
RG_DEV bool rg_closed(const RgCtx& c, int y, int x) {
    if (x < 1 || x > c.w - 2) return false;
    const uint8_t* row = c.cls + (size_t)y * c.W;
    const bool m1 = row[x - 1] == c.c, m2 = row[x] == c.c, m3 = row[x + 1] == c.c;
    const bool m0 = x >= 2 && row[x - 2] == c.c, m4 = x + 2 < c.w && row[x + 2] == c.c;
    return (m0 | m1 | m2) & (m1 | m2 | m3) & (m2 | m3 | m4);
}

// root of a; parents never exceed their children, so the walk is at most npix long
RG_DEV int rg_find(const RgLds& s, int a, int npix) {
    for (int it = 0; it < npix; ++it) {
        const int p = rg_ld(s.L + a);
        if (p == a) break;
        a = p;
    }
    return a;
}

// lock-free union: hang the larger root under the smaller one; a + b decreases with every retry
RG_DEV void rg_union(const RgLds& s, int a, int b, int npix) {
    for (unsigned it = 0; it < 2u * (unsigned)npix + 2u; ++it) {             // (unsigned: npix may be close to 2^31)
        a = rg_find(s, a, npix);
        b = rg_find(s, b, npix);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = rg_amin(s.L + a, b);
        if (old == a) return;
        a = old;
    }
    rg_aor(s.misc + RG_FAIL, RG_OVF_LABEL);
}

// component number of a mask pixel after rg_ph_assign: roots hold -2 - rank, the others their root
RG_DEV int rg_comp(const RgLds& s, int p) {
    const int l = s.L[p];
    return l < RG_BG ? -2 - l : -2 - s.L[l];
}

RG_DEV unsigned rg_hash(unsigned key) { return (key * 2654435761u) >> 21; }        // 11 bits: RG_HASH = 2048

// slot of `key`, inserted if absent; -1 (and the overflow bit) when the table is full
RG_DEV int rg_slot(const RgLds& s, unsigned key) {
    unsigned slot = rg_hash(key) & (RG_HASH - 1);
    for (int it = 0; it < RG_HASH; ++it) {
        const unsigned old = rg_acas(s.hk + slot, RG_EMPTY, key);
        if (old == RG_EMPTY) { rg_aadd(s.misc + RG_NPAIR, 1); return (int)slot; }
        if (old == key) return (int)slot;
        slot = (slot + 1) & (RG_HASH - 1);
    }
    rg_aor(s.misc + RG_FAIL, RG_OVF_PAIRS);
    return -1;
}

// ---- phases ------------------------------------------------------------------------------------------------------
RG_DEV void rg_ph_init(const RgCtx& c, const RgLds& s, int tid) {
    const int npix = c.h * c.w;
    for (int p = tid; p < npix; p += RG_THREADS) {
        const int y = p / c.w, x = p - y * c.w;
        s.L[p] = rg_closed(c, y, x) ? p : RG_BG;
    }
    for (int i = tid; i < RG_HASH; i += RG_THREADS) { s.hk[i] = RG_EMPTY; s.hn[i] = 0; s.hmn[i] = 65535; s.hmx[i] = 0; }
    if (tid < RG_MISC) s.misc[tid] = 0;
}

// every mask pixel with a mask pixel on its left points at it ...
RG_DEV void rg_ph_link_left(const RgCtx& c, const RgLds& s, int tid) {
    const int npix = c.h * c.w;
    for (int p = tid; p < npix; p += RG_THREADS) {
        const int x = p % c.w;
        if (x > 0 && rg_ld(s.L + p) != RG_BG && rg_ld(s.L + p - 1) != RG_BG) s.L[p] = p - 1;
    }
}

// ... and pointer jumping (ceil(log2 w) rounds) brings it to the start of its row run
RG_DEV void rg_ph_jump(const RgCtx& c, const RgLds& s, int tid) {
    const int npix = c.h * c.w;
    for (int p = tid; p < npix; p += RG_THREADS) {
        const int l = rg_ld(s.L + p);
        if (l != RG_BG) s.L[p] = rg_ld(s.L + l);
    }
}

// join the runs of neighbouring rows (a pixel whose left, upper and upper-left neighbours are all set adds nothing)
RG_DEV void rg_ph_union_up(const RgCtx& c, const RgLds& s, int tid) {
    const int npix = c.h * c.w;
    for (int p = c.w + tid; p < npix; p += RG_THREADS) {
        if (rg_ld(s.L + p) == RG_BG || rg_ld(s.L + p - c.w) == RG_BG) continue;
        const int x = p % c.w;
        if (x > 0 && rg_ld(s.L + p - 1) != RG_BG && rg_ld(s.L + p - c.w - 1) != RG_BG) continue;
        rg_union(s, p, p - c.w, npix);
    }
}

RG_DEV void rg_ph_flatten(const RgCtx& c, const RgLds& s, int tid) {
    const int npix = c.h * c.w;
    for (int p = tid; p < npix; p += RG_THREADS)
        if (rg_ld(s.L + p) != RG_BG) s.L[p] = rg_find(s, p, npix);
}

// rank the roots by linear index: lane t owns pixels [t * chunk, (t + 1) * chunk)
RG_DEV void rg_ph_count(const RgCtx& c, const RgLds& s, int tid) {
    const int npix = c.h * c.w, chunk = (npix + RG_THREADS - 1) / RG_THREADS;
    int n = 0;
    for (int i = 0; i < chunk; ++i) {
        const int p = tid * chunk + i;
        if (p < npix && s.L[p] == p) ++n;
    }
    s.scan[tid] = n;
}

RG_DEV void rg_ph_scan_parts(const RgCtx& c, const RgLds& s, int tid) {
    if (tid >= 32) return;
    int n = 0;
    for (int i = 0; i < RG_THREADS / 32; ++i) n += s.scan[tid * (RG_THREADS / 32) + i];
    s.part[tid] = n;
}

RG_DEV void rg_ph_scan_top(const RgCtx& c, const RgLds& s, int tid) {
    if (tid != 0) return;
    int run = 0;
    for (int i = 0; i < 32; ++i) { const int n = s.part[i]; s.part[i] = run; run += n; }
    s.misc[RG_NCOMP] = run;
    if (run > RG_MAXK) s.misc[RG_FAIL] |= RG_OVF_REGIONS;
}

RG_DEV void rg_ph_assign(const RgCtx& c, const RgLds& s, int tid) {
    const int npix = c.h * c.w, chunk = (npix + RG_THREADS - 1) / RG_THREADS, per = RG_THREADS / 32;
    int rank = s.part[tid / per];
    for (int i = (tid / per) * per; i < tid; ++i) rank += s.scan[i];
    for (int i = 0; i < chunk; ++i) {
        const int p = tid * chunk + i;
        if (p < npix && s.L[p] == p) {
            if (rank < RG_MAXK) {
                s.cfirst[rank] = p;
                s.cy0[rank] = c.h; s.cy1[rank] = -1; s.cx0[rank] = c.w; s.cx1[rank] = -1; s.ccnt[rank] = 0;
            }
            s.L[p] = -2 - rank;
            ++rank;
        }
    }
}

RG_DEV void rg_ph_stats(const RgCtx& c, const RgLds& s, int tid) {
    const int npix = c.h * c.w;
    for (int p = tid; p < npix; p += RG_THREADS) {
        if (s.L[p] == RG_BG) continue;
        const int k = rg_comp(s, p), y = p / c.w, x = p - y * c.w;
        rg_amin(s.cy0 + k, y); rg_amax(s.cy1 + k, y);
        rg_amin(s.cx0 + k, x); rg_amax(s.cx1 + k, x);
        rg_aadd(s.ccnt + k, 1);
    }
}

// n_under: by the line-id mask
RG_DEV void rg_ph_pairs_pix(const RgCtx& c, const RgLds& s, int tid) {
    const int npix = c.h * c.w;
    for (int p = tid; p < npix; p += RG_THREADS) {
        if (s.L[p] == RG_BG) continue;
        const int y = p / c.w, x = p - y * c.w;
        const int v = c.line[(size_t)y * c.W + x];
        if (v == 0) continue;
        if (v > c.n_lines) { rg_aor(s.misc + RG_FAIL, RG_OVF_LINES); continue; }
        const int slot = rg_slot(s, ((unsigned)rg_comp(s, p) << 16) | (unsigned)v);
        if (slot >= 0) rg_aadd(s.hn + slot, 1);
    }
}

// cp_min / cp_max: by the line's box, clipped to the document; one wavefront per line, its lanes over the box
RG_DEV void rg_ph_pairs_box(const RgCtx& c, const RgLds& s, int tid) {
    const int wv = tid >> 6, lane = tid & 63;
    for (int li = wv; li < c.n_lines; li += RG_THREADS / 64) {
        const int32_t* b = c.boxes + 4 * (size_t)li;
        const int x1 = b[0] > 0 ? b[0] : 0, y1 = b[1] > 0 ? b[1] : 0;
        const int x2 = b[2] < c.w ? b[2] : c.w, y2 = b[3] < c.h ? b[3] : c.h;
        if (x2 <= x1 || y2 <= y1) continue;
        const int bw = x2 - x1, area = bw * (y2 - y1);               // <= npix
        for (int i = lane; i < area; i += 64) {
            const int y = y1 + i / bw, x = x1 + i % bw, p = y * c.w + x;
            if (s.L[p] == RG_BG) continue;
            const int cp = c.chr[(size_t)y * c.W + x];
            if (cp == 0) continue;
            const int slot = rg_slot(s, ((unsigned)rg_comp(s, p) << 16) | (unsigned)(li + 1));
            if (slot >= 0) { rg_amin(s.hmn + slot, cp); rg_amax(s.hmx + slot, cp); }
        }
    }
}

// one compare-exchange step of the bitonic network over the RG_HASH entries (empty keys are the largest: they end up last)
RG_DEV void rg_ph_bitonic(const RgCtx& c, const RgLds& s, int tid, int k, int j) {
    const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), o = i | j;      // the pair (i, i + j) of lane tid
    const bool up = (i & k) == 0;
    const unsigned a = s.hk[i], b = s.hk[o];
    if ((a > b) == up) {
        s.hk[i] = b; s.hk[o] = a;
        int t;
        t = s.hn[i]; s.hn[i] = s.hn[o]; s.hn[o] = t;
        t = s.hmn[i]; s.hmn[i] = s.hmn[o]; s.hmn[o] = t;
        t = s.hmx[i]; s.hmx[i] = s.hmx[o]; s.hmx[o] = t;
    }
}

// reserve this class's slices of the document's lists: one 32-bit atomic each
RG_DEV void rg_ph_reserve(const RgCtx& c, const RgLds& s, int tid) {
    if (tid != 0) return;
    const int nc = s.misc[RG_NCOMP], np = s.misc[RG_NPAIR];
    const int roff = rg_aadd(c.hdr + 0, nc), poff = rg_aadd(c.hdr + 1, np);
    s.misc[RG_ROFF] = roff; s.misc[RG_POFF] = poff;
    if (roff + nc > c.cap_regions) s.misc[RG_FAIL] |= RG_OVF_REGIONS;
    if (poff + np > c.cap_pairs) s.misc[RG_FAIL] |= RG_OVF_PAIRS;
}

RG_DEV void rg_ph_write(const RgCtx& c, const RgLds& s, int tid) {
    const int nc = s.misc[RG_NCOMP], np = s.misc[RG_NPAIR], roff = s.misc[RG_ROFF], poff = s.misc[RG_POFF];
    for (int k = tid; k < nc; k += RG_THREADS) {
        int32_t* r = c.regions + (size_t)(roff + k) * RG_REGION_INTS;
        const int first = s.cfirst[k];
        r[0] = first / c.w; r[1] = first % c.w;
        r[2] = s.cy0[k]; r[3] = s.cy1[k] + 1; r[4] = s.cx0[k]; r[5] = s.cx1[k] + 1;
        r[6] = s.ccnt[k]; r[7] = c.c;
    }
    for (int i = tid; i < np; i += RG_THREADS) {
        int32_t* q = c.pairs + (size_t)(poff + i) * RG_PAIR_INTS;
        q[0] = (int32_t)s.hk[i]; q[1] = s.hn[i]; q[2] = s.hmn[i]; q[3] = s.hmx[i];
    }
    if (tid == 0) {
        int32_t* hd = c.hdr + 4 * c.c;
        hd[0] = roff; hd[1] = nc; hd[2] = poff; hd[3] = np;
    }
}

// ---- the scored form's phases, behind rg_ph_write ------------------------------------------------------------------
// q(p) = rint(p * 65536): the scale is a power of two, so the product is exact and the conversion is the only rounding
RG_DEV int rg_quant(float p) { return rg_rint(p * 65536.0f); }

RG_DEV void rg_ph_score_zero(const RgCtx& c, const RgLds& s, int tid) {
    const int nc = s.misc[RG_NCOMP];
    for (int k = tid; k < nc; k += RG_THREADS) s.sum[k] = 0;
}

// lane t owns pixels [t * chunk, (t + 1) * chunk) as in rg_ph_count: it sums a run of one component locally and adds the run's
// sum when the component changes.  A component of RG_LARGE_MAXPIX pixels at p = 1 sums to less than 2^47.
RG_DEV void rg_ph_score_sum(const RgCtx& c, const RgLds& s, int tid) {
    const int npix = c.h * c.w, chunk = (npix + RG_THREADS - 1) / RG_THREADS;
    int cur = -1;
    long long run = 0;
    for (int i = 0; i < chunk; ++i) {
        const int p = tid * chunk + i;
        if (p >= npix) break;
        if (s.L[p] == RG_BG) continue;
        const int k = rg_comp(s, p), y = p / c.w, x = p - y * c.w;
        if (k != cur) {
            if (cur >= 0) rg_aadd64(s.sum + cur, run);
            cur = k; run = 0;
        }
        run += rg_quant(c.probs[((size_t)y * c.W + x) * c.n_class + c.c]);
    }
    if (cur >= 0) rg_aadd64(s.sum + cur, run);
}

// every row this class reserved, and no other
RG_DEV void rg_ph_score_write(const RgCtx& c, const RgLds& s, int tid) {
    const int nc = s.misc[RG_NCOMP], roff = s.misc[RG_ROFF];
    for (int k = tid; k < nc; k += RG_THREADS) c.scores[roff + k] = s.sum[k];
}

// -> the overflow bits of this (document, class); 0 = its slices and its header row are written
template <bool SCORED>
RG_DEV int rg_body(const RgCtx& c, const RgLds& s) {
    RG_PHASE(rg_ph_init);
    RG_PHASE(rg_ph_link_left);
    for (int span = 1; span < c.w; span *= 2) RG_PHASE(rg_ph_jump);
    RG_PHASE(rg_ph_union_up);
    RG_CHECK();
    RG_PHASE(rg_ph_flatten);
    RG_PHASE(rg_ph_count);
    RG_PHASE(rg_ph_scan_parts);
    RG_PHASE(rg_ph_scan_top);
    RG_CHECK();
    RG_PHASE(rg_ph_assign);
    RG_PHASE(rg_ph_stats);
    RG_PHASE(rg_ph_pairs_pix);
    RG_PHASE(rg_ph_pairs_box);
    RG_CHECK();
    if (s.misc[RG_NPAIR] > 0)
        for (int k = 2; k <= RG_HASH; k *= 2)
            for (int j = k / 2; j >= 1; j /= 2) RG_PHASE(rg_ph_bitonic, k, j);
    RG_PHASE(rg_ph_reserve);
    RG_CHECK();
    RG_PHASE(rg_ph_write);
    if constexpr (SCORED) {
        RG_PHASE(rg_ph_score_zero);
        RG_PHASE(rg_ph_score_sum);
        RG_PHASE(rg_ph_score_write);
    }
    return 0;
}

// the checks that need no LDS: a document this form does not hold, an extent outside the canvas, a line list too long
RG_DEV int rg_precheck(int h, int w, int H, int W, int n_lines, int64_t max_pixels) {
    if (h < 1 || w < 1 || h > H || w > W || (int64_t)h * w > max_pixels) return RG_OVF_PIXELS;
    if (n_lines < 0 || n_lines > RG_MAXLINES) return RG_OVF_LINES;
    return 0;
}

// the (document b, class cc) of a launch
RG_DEV void rg_ctx(RgCtx& c, int b, int cc, const uint8_t* argmax, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes,
                   const int32_t* box_off, const int32_t* extent, int H, int W, int n_class, int32_t* header, int32_t* regions,
                   int cap_regions, int32_t* pairs, int cap_pairs) {
    const size_t plane = (size_t)b * H * W;
    c.cls = argmax + plane; c.line = line_ids + plane; c.chr = char_pos + plane;
    c.boxes = boxes + 4 * (size_t)box_off[b]; c.n_lines = box_off[b + 1] - box_off[b];
    c.h = extent ? extent[2 * b] : H; c.w = extent ? extent[2 * b + 1] : W; c.W = W; c.c = cc;
    c.hdr = header + 4 * (size_t)b * n_class;
    c.regions = regions + (size_t)b * cap_regions * RG_REGION_INTS; c.cap_regions = cap_regions;
    c.pairs = pairs + (size_t)b * cap_pairs * RG_PAIR_INTS; c.cap_pairs = cap_pairs;
}

// ... and what the scored form reads and writes besides
RG_DEV void rg_ctx_scores(RgCtx& c, int b, const float* probs, int H, int W, int n_class, int64_t* scores, int cap_regions) {
    c.probs = probs + (size_t)b * H * W * n_class; c.n_class = n_class;
    c.scores = scores + (size_t)b * cap_regions;
}

// ---- the large form ------------------------------------------------------------------------------------------------
// The documents of one launch and their shares of the workspace.  Class cc of document doc[i] labels in
// workspace[off[i] + (cc - 2) * h * w ..); a share that is too small for that is the document's RG_OVF_PIXELS.
struct RgLargeDocs { int64_t off[RG_LARGE_DOCS]; int64_t share[RG_LARGE_DOCS]; int32_t doc[RG_LARGE_DOCS]; };

// what the host can say about the list; `ext` = the extents when the host can read them (ext_known), NULL with ext_known for a
// dense batch.  -> NULL or the complaint
static inline const char* rg_large_args(int B, int H, int W, int n_class, const int32_t* docs, int n_docs, const int64_t* ws_off,
                                        int64_t workspace_ints, const int32_t* ext, int ext_known) {
    if (!docs || !ws_off) return "null document list";
    if (n_docs < 1 || n_docs > B) return "n_docs must be in [1, B]";
    if (workspace_ints < 0) return "negative workspace size";
    for (int i = 0; i < n_docs; ++i) {
        if (docs[i] < 0 || docs[i] >= B) return "a listed document is outside [0, B)";
        for (int j = 0; j < i; ++j) if (docs[j] == docs[i]) return "a document is listed twice";
        const int64_t end = i + 1 < n_docs ? ws_off[i + 1] : workspace_ints;
        if (ws_off[i] < 0 || end < ws_off[i] || end > workspace_ints) return "workspace offsets must increase within the workspace";
        if (ext_known) {
            const int64_t h = ext ? ext[2 * docs[i]] : H, w = ext ? ext[2 * docs[i] + 1] : W;
            if (h >= 1 && w >= 1 && h <= H && w <= W && (n_class - 2) * h * w > end - ws_off[i])
                return "a workspace share is smaller than (n_class - 2) * h * w";
        }
    }
    return 0;
}

RG_DEV int64_t rg_large_pixels(int64_t share, int n_class) {
    const int64_t fit = share / (n_class - 2);
    return fit < RG_LARGE_MAXPIX ? fit : RG_LARGE_MAXPIX;
}

#ifdef MSAU_REGIONS_CPU
// the launch, lane by lane on the host (probs and scores: the scored form's, NULL otherwise)
template <bool SCORED>
static int rg_cpu_lds(const uint8_t* argmax, const float* probs, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes,
                      const int32_t* box_off, const int32_t* extent, int B, int H, int W, int n_class, int32_t* header, int32_t* regions,
                      int cap_regions, int32_t* pairs, int cap_pairs, int64_t* scores, int32_t* overflow) {
    int* lds = (int*)malloc(sizeof(int) * RG_LDS_INTS);
    if (!lds) return 1;
    memset(header, 0, sizeof(int32_t) * 4 * (size_t)B * n_class);
    memset(overflow, 0, sizeof(int32_t) * B);
    for (int b = 0; b < B; ++b)
        for (int cc = 2; cc < n_class; ++cc) {
            RgCtx c;
            rg_ctx(c, b, cc, argmax, line_ids, char_pos, boxes, box_off, extent, H, W, n_class, header, regions, cap_regions, pairs, cap_pairs);
            if (SCORED) rg_ctx_scores(c, b, probs, H, W, n_class, scores, cap_regions);
            RgLds s;
            rg_carve(s, lds, lds + RG_MAXPIX);
            int f = rg_precheck(c.h, c.w, H, W, c.n_lines, RG_MAXPIX);
            if (!f) f = rg_body<SCORED>(c, s);
            overflow[b] |= f;
        }
    free(lds);
    return 0;
}
// the large launch, lane by lane on the host; 2 = refused arguments
template <bool SCORED>
static int rg_cpu_large(const uint8_t* argmax, const float* probs, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes,
                        const int32_t* box_off, const int32_t* extent, int B, int H, int W, int n_class, const int32_t* docs, int n_docs,
                        const int64_t* ws_off, int32_t* workspace, int64_t workspace_ints, int32_t* header, int32_t* regions,
                        int cap_regions, int32_t* pairs, int cap_pairs, int64_t* scores, int32_t* overflow) {
    if (!(argmax && line_ids && char_pos && boxes && box_off && workspace && header && regions && pairs && overflow)) return 2;
    if (SCORED && !(probs && scores)) return 2;
    if (!(B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && n_class >= 1 && n_class <= 255 && cap_regions >= 1 && cap_pairs >= 1)) return 2;
    if (rg_large_args(B, H, W, n_class, docs, n_docs, ws_off, workspace_ints, extent, 1)) return 2;
    int* lds = (int*)malloc(sizeof(int) * RG_TABLE_INTS);
    if (!lds) return 1;
    for (int i = 0; i < n_docs; ++i) {
        const int b = docs[i];
        memset(header + 4 * (size_t)b * n_class, 0, sizeof(int32_t) * 4 * n_class);
        overflow[b] = 0;
        const int64_t share = (i + 1 < n_docs ? ws_off[i + 1] : workspace_ints) - ws_off[i];
        for (int cc = 2; cc < n_class; ++cc) {
            RgCtx c;
            rg_ctx(c, b, cc, argmax, line_ids, char_pos, boxes, box_off, extent, H, W, n_class, header, regions, cap_regions, pairs, cap_pairs);
            if (SCORED) rg_ctx_scores(c, b, probs, H, W, n_class, scores, cap_regions);
            RgLds s;
            int f = rg_precheck(c.h, c.w, H, W, c.n_lines, rg_large_pixels(share, n_class));
            if (!f) {
                rg_carve(s, workspace + ws_off[i] + (int64_t)(cc - 2) * c.h * c.w, lds);
                f = rg_body<SCORED>(c, s);
            }
            overflow[b] |= f;
        }
    }
    free(lds);
    return 0;
}
// same arguments as msau_kv_regions / msau_kv_regions_large / their scored forms without the stream
extern "C" int msau_kv_regions_cpu(const uint8_t* argmax, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes,
                                   const int32_t* box_off, const int32_t* extent, int B, int H, int W, int n_class, int32_t* header,
                                   int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int32_t* overflow) {
    return rg_cpu_lds<false>(argmax, 0, line_ids, char_pos, boxes, box_off, extent, B, H, W, n_class, header, regions, cap_regions, pairs,
                             cap_pairs, 0, overflow);
}
extern "C" int msau_kv_regions_scored_cpu(const uint8_t* argmax, const float* probs, const uint16_t* line_ids, const uint16_t* char_pos,
                                          const int32_t* boxes, const int32_t* box_off, const int32_t* extent, int B, int H, int W,
                                          int n_class, int32_t* header, int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs,
                                          int64_t* scores, int32_t* overflow) {
    if (!(probs && scores)) return 2;
    return rg_cpu_lds<true>(argmax, probs, line_ids, char_pos, boxes, box_off, extent, B, H, W, n_class, header, regions, cap_regions, pairs,
                            cap_pairs, scores, overflow);
}
extern "C" int msau_kv_regions_large_cpu(const uint8_t* argmax, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes,
                                         const int32_t* box_off, const int32_t* extent, int B, int H, int W, int n_class,
                                         const int32_t* docs, int n_docs, const int64_t* ws_off, int32_t* workspace, int64_t workspace_ints,
                                         int32_t* header, int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int32_t* overflow) {
    return rg_cpu_large<false>(argmax, 0, line_ids, char_pos, boxes, box_off, extent, B, H, W, n_class, docs, n_docs, ws_off, workspace,
                               workspace_ints, header, regions, cap_regions, pairs, cap_pairs, 0, overflow);
}
extern "C" int msau_kv_regions_large_scored_cpu(const uint8_t* argmax, const float* probs, const uint16_t* line_ids, const uint16_t* char_pos,
                                                const int32_t* boxes, const int32_t* box_off, const int32_t* extent, int B, int H, int W,
                                                int n_class, const int32_t* docs, int n_docs, const int64_t* ws_off, int32_t* workspace,
                                                int64_t workspace_ints, int32_t* header, int32_t* regions, int cap_regions, int32_t* pairs,
                                                int cap_pairs, int64_t* scores, int32_t* overflow) {
    return rg_cpu_large<true>(argmax, probs, line_ids, char_pos, boxes, box_off, extent, B, H, W, n_class, docs, n_docs, ws_off, workspace,
                              workspace_ints, header, regions, cap_regions, pairs, cap_pairs, scores, overflow);
}
extern "C" int msau_kv_regions_limits(int32_t* out) {
    out[0] = RG_MAXPIX; out[1] = RG_MAXK; out[2] = RG_HASH; out[3] = RG_REGION_INTS; out[4] = RG_PAIR_INTS; out[5] = RG_MAXLINES;
    return 0;
}
#else

// one workgroup of the LDS form: (document blockIdx.y, class 2 + blockIdx.x), the labels and the tables in `lds`
template <bool SCORED>
RG_DEV void rg_lds_form(int* lds, const uint8_t* argmax, const float* probs, const uint16_t* line_ids, const uint16_t* char_pos,
                        const int32_t* boxes, const int32_t* box_off, const int32_t* extent, int H, int W, int n_class, int32_t* header,
                        int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int64_t* scores, int32_t* overflow) {
    const int b = blockIdx.y;
    RgCtx c;
    rg_ctx(c, b, 2 + (int)blockIdx.x, argmax, line_ids, char_pos, boxes, box_off, extent, H, W, n_class, header, regions, cap_regions, pairs, cap_pairs);
    if constexpr (SCORED) rg_ctx_scores(c, b, probs, H, W, n_class, scores, cap_regions);
    RgLds s;
    rg_carve(s, lds, lds + RG_MAXPIX);
    int f = rg_precheck(c.h, c.w, H, W, c.n_lines, RG_MAXPIX);     // uniform over the workgroup, like every exit of rg_body
    if (!f) f = rg_body<SCORED>(c, s);
    if (f && threadIdx.x == 0) atomicOr(overflow + b, f);
}

__global__ void __launch_bounds__(RG_THREADS)
kv_regions_kernel(const uint8_t* argmax, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes, const int32_t* box_off,
                  const int32_t* extent, int H, int W, int n_class, int32_t* header, int32_t* regions, int cap_regions, int32_t* pairs,
                  int cap_pairs, int32_t* overflow) {
    extern __shared__ int rg_lds[];
    rg_lds_form<false>(rg_lds, argmax, nullptr, line_ids, char_pos, boxes, box_off, extent, H, W, n_class, header, regions, cap_regions, pairs,
                       cap_pairs, nullptr, overflow);
}

__global__ void __launch_bounds__(RG_THREADS)
kv_regions_scored_kernel(const uint8_t* argmax, const float* probs, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes,
                         const int32_t* box_off, const int32_t* extent, int H, int W, int n_class, int32_t* header, int32_t* regions,
                         int cap_regions, int32_t* pairs, int cap_pairs, int64_t* scores, int32_t* overflow) {
    extern __shared__ int rg_lds[];
    rg_lds_form<true>(rg_lds, argmax, probs, line_ids, char_pos, boxes, box_off, extent, H, W, n_class, header, regions, cap_regions, pairs,
                      cap_pairs, scores, overflow);
}

// The large form: the labels of (document ld.doc[blockIdx.y], class 2 + blockIdx.x) in that pair's own h * w int32 of the
// workspace, the tables in LDS, the phases of rg_body as they are.  Only this workgroup touches its share, and only between its
// own barriers: see DESIGN.md 5b for why plain accesses and rg_ld's L2 loads see what they must.
template <bool SCORED>
RG_DEV void rg_large_form(int* tables, const uint8_t* argmax, const float* probs, const uint16_t* line_ids, const uint16_t* char_pos,
                          const int32_t* boxes, const int32_t* box_off, const int32_t* extent, int H, int W, int n_class,
                          const RgLargeDocs& ld, int32_t* workspace, int32_t* header, int32_t* regions, int cap_regions, int32_t* pairs,
                          int cap_pairs, int64_t* scores, int32_t* overflow) {
    const int i = blockIdx.y, b = ld.doc[i];
    RgCtx c;
    rg_ctx(c, b, 2 + (int)blockIdx.x, argmax, line_ids, char_pos, boxes, box_off, extent, H, W, n_class, header, regions, cap_regions, pairs, cap_pairs);
    if constexpr (SCORED) rg_ctx_scores(c, b, probs, H, W, n_class, scores, cap_regions);
    RgLds s;
    int f = rg_precheck(c.h, c.w, H, W, c.n_lines, rg_large_pixels(ld.share[i], n_class));
    if (!f) {
        rg_carve(s, workspace + ld.off[i] + (int64_t)blockIdx.x * c.h * c.w, tables);
        f = rg_body<SCORED>(c, s);
    }
    if (f && threadIdx.x == 0) atomicOr(overflow + b, f);
}

__global__ void __launch_bounds__(RG_THREADS)
kv_regions_large_kernel(const uint8_t* argmax, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes, const int32_t* box_off,
                        const int32_t* extent, int H, int W, int n_class, RgLargeDocs ld, int32_t* workspace, int32_t* header,
                        int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int32_t* overflow) {
    __shared__ int rg_tables[RG_TABLE_INTS];
    rg_large_form<false>(rg_tables, argmax, nullptr, line_ids, char_pos, boxes, box_off, extent, H, W, n_class, ld, workspace, header, regions,
                         cap_regions, pairs, cap_pairs, nullptr, overflow);
}

__global__ void __launch_bounds__(RG_THREADS)
kv_regions_large_scored_kernel(const uint8_t* argmax, const float* probs, const uint16_t* line_ids, const uint16_t* char_pos,
                               const int32_t* boxes, const int32_t* box_off, const int32_t* extent, int H, int W, int n_class, RgLargeDocs ld,
                               int32_t* workspace, int32_t* header, int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs,
                               int64_t* scores, int32_t* overflow) {
    __shared__ __attribute__((aligned(8))) int rg_tables[RG_TABLE_INTS];      // (the 64-bit sums lie over two of the tables)
    rg_large_form<true>(rg_tables, argmax, probs, line_ids, char_pos, boxes, box_off, extent, H, W, n_class, ld, workspace, header, regions,
                        cap_regions, pairs, cap_pairs, scores, overflow);
}

// the listed documents' header rows and overflow words, as msau_kv_regions leaves them before its launch
__global__ void kv_regions_large_reset_kernel(RgLargeDocs ld, int n_class, int32_t* header, int32_t* overflow) {
    const int b = ld.doc[blockIdx.x];
    for (int i = threadIdx.x; i < 4 * n_class; i += blockDim.x) header[4 * (size_t)b * n_class + i] = 0;
    if (threadIdx.x == 0) overflow[b] = 0;
}

extern "C" int msau_kv_regions_limits(int32_t* out) {
    MSAU_CHECK_ARG(out, "kv_regions_limits: null");
    out[0] = RG_MAXPIX; out[1] = RG_MAXK; out[2] = RG_HASH; out[3] = RG_REGION_INTS; out[4] = RG_PAIR_INTS; out[5] = RG_MAXLINES;
    return 0;
}

// msau_kv_regions (`who` = "kv_regions") and its scored form
template <bool SCORED>
static int rg_launch_lds(const char* who, void* stream, const uint8_t* argmax, const float* probs, const uint16_t* line_ids,
                         const uint16_t* char_pos, const int32_t* boxes, const int32_t* box_off, const int32_t* extent, int B, int H, int W,
                         int n_class, int32_t* header, int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int64_t* scores,
                         int32_t* overflow) {
    MSAU_CHECK_ARG(argmax && line_ids && char_pos && boxes && box_off && header && regions && pairs && overflow, "%s: null pointer", who);
    MSAU_CHECK_ARG(!SCORED || (probs && scores), "%s: null probs or scores", who);
    MSAU_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "%s: bad shape B = %d, H = %d, W = %d", who, B, H, W);
    MSAU_CHECK_ARG(n_class >= 1 && n_class <= 255, "%s: n_class = %d, must be in [1, 255]", who, n_class);
    MSAU_CHECK_ARG(cap_regions >= 1 && cap_pairs >= 1 && cap_regions < (1 << 24) && cap_pairs < (1 << 24), "%s: bad capacities", who);
    static_assert(sizeof(int) * RG_LDS_INTS <= MSAU_LDS_LIMIT, "kv_regions: the tables must fit the LDS");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(header, 0, sizeof(int32_t) * 4 * (size_t)B * n_class, s);
    if (e == hipSuccess) e = hipMemsetAsync(overflow, 0, sizeof(int32_t) * (size_t)B, s);
    if (e != hipSuccess) return msau_set_error(MSAU_ERR_HIP, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    if (n_class < 3) return 0;
    const void* kern = SCORED ? reinterpret_cast<const void*>(&kv_regions_scored_kernel) : reinterpret_cast<const void*>(&kv_regions_kernel);
    static bool attr_set = false;                                  // (one per form)
    if (!attr_set) {
        e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, MSAU_LDS_LIMIT);
        if (e != hipSuccess) return msau_set_error(MSAU_ERR_HIP, "%s: hipFuncSetAttribute: %s", who, hipGetErrorString(e));
        attr_set = true;
    }
    if constexpr (SCORED)
        hipLaunchKernelGGL(kv_regions_scored_kernel, dim3(n_class - 2, B), dim3(RG_THREADS), sizeof(int) * RG_LDS_INTS, s, argmax, probs, line_ids,
                           char_pos, boxes, box_off, extent, H, W, n_class, header, regions, cap_regions, pairs, cap_pairs, scores, overflow);
    else
        hipLaunchKernelGGL(kv_regions_kernel, dim3(n_class - 2, B), dim3(RG_THREADS), sizeof(int) * RG_LDS_INTS, s, argmax, line_ids, char_pos, boxes,
                           box_off, extent, H, W, n_class, header, regions, cap_regions, pairs, cap_pairs, overflow);
    MSAU_CHECK_LAUNCH(who);
    return 0;
}

// msau_kv_regions_large (`who` = "kv_regions_large") and its scored form
template <bool SCORED>
static int rg_launch_large(const char* who, void* stream, const uint8_t* argmax, const float* probs, const uint16_t* line_ids,
                           const uint16_t* char_pos, const int32_t* boxes, const int32_t* box_off, const int32_t* extent, int B, int H, int W,
                           int n_class, const int32_t* docs, int n_docs, const int64_t* ws_off, int32_t* workspace, int64_t workspace_ints,
                           int32_t* header, int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int64_t* scores,
                           int32_t* overflow) {
    MSAU_CHECK_ARG(argmax && line_ids && char_pos && boxes && box_off && workspace && header && regions && pairs && overflow,
                   "%s: null pointer", who);
    MSAU_CHECK_ARG(!SCORED || (probs && scores), "%s: null probs or scores", who);
    MSAU_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "%s: bad shape B = %d, H = %d, W = %d", who, B, H, W);
    MSAU_CHECK_ARG(n_class >= 1 && n_class <= 255, "%s: n_class = %d, must be in [1, 255]", who, n_class);
    MSAU_CHECK_ARG(cap_regions >= 1 && cap_pairs >= 1 && cap_regions < (1 << 24) && cap_pairs < (1 << 24), "%s: bad capacities", who);
    const char* bad = rg_large_args(B, H, W, n_class, docs, n_docs, ws_off, workspace_ints, nullptr, extent == nullptr);
    MSAU_CHECK_ARG(!bad, "%s: %s", who, bad);
    static_assert(sizeof(int) * RG_TABLE_INTS <= 64 * 1024, "kv_regions_large: the tables are a static LDS array");
    static_assert(sizeof(RgLargeDocs) <= 1024, "kv_regions_large: the document list is a kernel argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int k = 0; k < n_docs; k += RG_LARGE_DOCS) {
        const int n = n_docs - k < RG_LARGE_DOCS ? n_docs - k : RG_LARGE_DOCS;
        RgLargeDocs ld = {};
        for (int i = 0; i < n; ++i) {
            ld.doc[i] = docs[k + i];
            ld.off[i] = ws_off[k + i];
            ld.share[i] = (k + i + 1 < n_docs ? ws_off[k + i + 1] : workspace_ints) - ws_off[k + i];
        }
        hipLaunchKernelGGL(kv_regions_large_reset_kernel, dim3(n), dim3(256), 0, s, ld, n_class, header, overflow);
        MSAU_CHECK_LAUNCH("kv_regions_large (reset)");
        if (n_class < 3) continue;
        if constexpr (SCORED)
            hipLaunchKernelGGL(kv_regions_large_scored_kernel, dim3(n_class - 2, n), dim3(RG_THREADS), 0, s, argmax, probs, line_ids, char_pos, boxes,
                               box_off, extent, H, W, n_class, ld, workspace, header, regions, cap_regions, pairs, cap_pairs, scores, overflow);
        else
            hipLaunchKernelGGL(kv_regions_large_kernel, dim3(n_class - 2, n), dim3(RG_THREADS), 0, s, argmax, line_ids, char_pos, boxes, box_off,
                               extent, H, W, n_class, ld, workspace, header, regions, cap_regions, pairs, cap_pairs, overflow);
        MSAU_CHECK_LAUNCH(who);
    }
    return 0;
}

extern "C" int msau_kv_regions(void* stream, const uint8_t* argmax, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes,
                               const int32_t* box_off, const int32_t* extent, int B, int H, int W, int n_class, int32_t* header,
                               int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int32_t* overflow) {
    return rg_launch_lds<false>("kv_regions", stream, argmax, nullptr, line_ids, char_pos, boxes, box_off, extent, B, H, W, n_class, header,
                                regions, cap_regions, pairs, cap_pairs, nullptr, overflow);
}

extern "C" int msau_kv_regions_scored(void* stream, const uint8_t* argmax, const float* probs, const uint16_t* line_ids,
                                      const uint16_t* char_pos, const int32_t* boxes, const int32_t* box_off, const int32_t* extent, int B,
                                      int H, int W, int n_class, int32_t* header, int32_t* regions, int cap_regions, int32_t* pairs,
                                      int cap_pairs, int64_t* scores, int32_t* overflow) {
    return rg_launch_lds<true>("kv_regions_scored", stream, argmax, probs, line_ids, char_pos, boxes, box_off, extent, B, H, W, n_class, header,
                               regions, cap_regions, pairs, cap_pairs, scores, overflow);
}

extern "C" int msau_kv_regions_large(void* stream, const uint8_t* argmax, const uint16_t* line_ids, const uint16_t* char_pos, const int32_t* boxes,
                                     const int32_t* box_off, const int32_t* extent, int B, int H, int W, int n_class, const int32_t* docs,
                                     int n_docs, const int64_t* ws_off, int32_t* workspace, int64_t workspace_ints, int32_t* header,
                                     int32_t* regions, int cap_regions, int32_t* pairs, int cap_pairs, int32_t* overflow) {
    return rg_launch_large<false>("kv_regions_large", stream, argmax, nullptr, line_ids, char_pos, boxes, box_off, extent, B, H, W, n_class, docs,
                                  n_docs, ws_off, workspace, workspace_ints, header, regions, cap_regions, pairs, cap_pairs, nullptr, overflow);
}

extern "C" int msau_kv_regions_large_scored(void* stream, const uint8_t* argmax, const float* probs, const uint16_t* line_ids,
                                            const uint16_t* char_pos, const int32_t* boxes, const int32_t* box_off, const int32_t* extent,
                                            int B, int H, int W, int n_class, const int32_t* docs, int n_docs, const int64_t* ws_off,
                                            int32_t* workspace, int64_t workspace_ints, int32_t* header, int32_t* regions, int cap_regions,
                                            int32_t* pairs, int cap_pairs, int64_t* scores, int32_t* overflow) {
    return rg_launch_large<true>("kv_regions_large_scored", stream, argmax, probs, line_ids, char_pos, boxes, box_off, extent, B, H, W, n_class,
                                 docs, n_docs, ws_off, workspace, workspace_ints, header, regions, cap_regions, pairs, cap_pairs, scores, overflow);
}
#endif

