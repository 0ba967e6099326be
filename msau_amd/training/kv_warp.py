"""The generator's affine and rotation augmentation of a key-value training document (data_generator/data_generator_text.py:303-344,
utils/image_util.py:38-55), computed from the id canvas and the two label canvases instead of from one-hot planes.

The generator concatenates the three one-hot maps x 255 as uint8 [h, w, n_token + 2 n_class], warps every plane with a cubic
spline (`scipy.ndimage.affine_transform` / `rotate`: order 3, mode "constant", cval 0), thresholds every plane at > 64 -- the
input is then multi-hot or zero-hot -- and reads a label off every target: 1 if channel 1 is set, else the smallest set channel
>= 2, else 0.  Per plane that is a closed form ("Warps"):

    (sy, sx) = off + M (oy, ox) in float64, (row, col) order; outside [0, h-1] x [0, w-1] every plane is 0
    taps q = floor(s) - 1 .. floor(s) + 2 per axis with the cubic B-spline's weights, reflected by whole-sample mirror
    coefficients = the mirror-boundary prefilter of the plane (scipy does not pad for mode "constant"); an axis of length 1: c = I
    grey = clamp(rint(255 S)), S the separable sum over the plane; the plane is set iff grey > 64, i.e. iff 255 S > 64.5

so the value of plane c is  S_c = sum_{j,i} wy[j] wx[i] [canvas(j, i) == c]  and no one-hot plane is needed.  `warp_host` is that
statement in float64 (the prefilter as the exact inverse of the B-spline's collocation matrix): what the kernel of csrc/warp.hip
(`msau_kv_warp_train`) is tested against, and the fallback for a document the kernel flags.  `warp_train_device` is the launch.

The generator's third augmentation, `elastic_transform` (utils/image_util.py:58-90), is the second half of this file: `Elastic`,
`elastic_field`, the statement `elastic_values` / `elastic_host` and the launch `elastic_train_device` (`msau_kv_elastic_train`)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

THRESHOLD = 64.5                    # grey > 64 after rint <=> 255 S > 64.5 (rint(64.5) is 64: half to even)
WARP_TILE = 16                      # output pixels per side of a workgroup's tile (csrc/warp.hip: WP_TILE)


@dataclass
class Warp:
    """output pixel (oy, ox) reads the source at offset + matrix @ (oy, ox), as `scipy.ndimage.affine_transform` takes them"""
    matrix: np.ndarray                  # float64 [2, 2]
    offset: np.ndarray                  # float64 [2]
    out_shape: Tuple[int, int]          # (ho, wo)

    def __post_init__(self):
        self.matrix = np.ascontiguousarray(self.matrix, dtype=np.float64).reshape(2, 2)
        self.offset = np.ascontiguousarray(self.offset, dtype=np.float64).reshape(2)
        self.out_shape = (int(self.out_shape[0]), int(self.out_shape[1]))

    def record(self) -> np.ndarray:
        """the 6 doubles the kernel takes: m00, m01, m10, m11, off0, off1"""
        return np.concatenate([self.matrix.reshape(4), self.offset])


def identity_warp(shape) -> Warp:
    return Warp(np.eye(2), np.zeros(2), (int(shape[0]), int(shape[1])))


def affine_points(shape) -> np.ndarray:
    """the three float32 (row, col) points `affine_warp` moves: around shape // 2 at +- min(shape) // 3"""
    center = np.float32(shape[:2]) // 2
    square = min(shape[:2]) // 3
    return np.float32([center + square, [center[0] + square, center[1] - square], center - square])


def affine_warp(shape, affine_value: float, rs: np.random.RandomState) -> Warp:
    """`image_util.affine_transform`'s random map for a document of `shape`: three points around the centre, each moved by six draws
    of uniform(-a, a), a = min(shape) * affine_value; the affine map that takes the points to the moved ones (least squares, which
    is the unique map through the three pairs unless the points coincide: min(shape) < 3), rounded to float32 as the generator
    rounds it and widened again.  The generator draws from an unseedable `RandomState(None)`; here the draws come from `rs`, which
    `KVTrainBatches` seeds from its own generator, so a seeded run is reproducible.  The output has the input's shape."""
    shape = (int(shape[0]), int(shape[1]))
    alpha = min(shape) * affine_value
    pts1 = affine_points(shape)
    pts2 = pts1 + rs.uniform(-alpha, alpha, size=pts1.shape).astype(np.float32)
    A, b = [], []
    for (r, c), (tr, tc) in zip(pts1.astype(np.float64), pts2.astype(np.float64)):
        A += [[r, 0, c, 0, 1, 0], [0, r, 0, c, 0, 1]]
        b += [tr, tc]
    a0, a1, a2, a3, a4, a5 = np.linalg.lstsq(np.array(A), np.array(b), rcond=None)[0]
    m = np.float32([[a0, a2, a4], [a1, a3, a5]]).astype(np.float64)
    return Warp(m[:, :2], m[:, 2], shape)


def rotate_warp(shape, angle: float) -> Warp:
    """`scipy.ndimage.rotate(planes, angle)` with reshape=True as the affine map it hands on: the matrix [[cos, sin], [-sin, cos]]
    (degrees, scipy's cosdg / sindg), the output shape the extent of the rotated corner box + 0.5, truncated, and the offset that
    takes the output's centre to the input's."""
    from scipy import special
    shape = (int(shape[0]), int(shape[1]))
    c, s = float(special.cosdg(angle)), float(special.sindg(angle))
    m = np.array([[c, s], [-s, c]], dtype=np.float64)
    h, w = shape
    bounds = m @ np.array([[0, 0, h, h], [0, w, 0, w]], dtype=np.float64)
    out = (np.ptp(bounds, axis=1) + 0.5).astype(int)
    offset = (np.array(shape, dtype=np.float64) - 1) / 2 - m @ ((out - 1) / 2)
    return Warp(m, offset, (int(out[0]), int(out[1])))


def mod90_angle(angle: float) -> float:
    """the generator's `rotateMod90` mapping of its uniform(-20, 20) draw, as written there: below 0 and below 45 both give -45, so
    it always yields -45 degrees (the 45 and 90 branches cannot be reached)"""
    if angle < 0:
        return -45.0
    if angle < 45:
        return -45.0
    return 45.0 if angle < 90.0 else 90.0


# ---- the statement ------------------------------------------------------------------------------------------------------------------
def _prefilter(n: int) -> np.ndarray:
    """[n, n]: spline coefficients from samples under whole-sample mirror, the inverse of the collocation matrix (1/6, 4/6, 1/6) whose
    first and last rows fold the mirrored neighbour onto the inner one.  Equal to sum_k sqrt(3) z^|k| I_m(q - k), z = sqrt(3) - 2."""
    if n == 1:
        return np.ones((1, 1))
    m = np.zeros((n, n))
    i = np.arange(n)
    m[i, i] = 4 / 6
    m[i[:-1], i[:-1] + 1] += 1 / 6
    m[i[1:], i[1:] - 1] += 1 / 6
    m[0, 1] = m[n - 1, n - 2] = 2 / 6
    return np.linalg.inv(m)


def _mirror(q: np.ndarray, n: int) -> np.ndarray:
    if n == 1:
        return np.zeros_like(q)
    q = np.mod(q, 2 * (n - 1))
    return np.where(q > n - 1, 2 * (n - 1) - q, q)


def _taps(s: np.ndarray, n: int):
    """-> (indices int [4, N], weights float64 [4, N]) of the four taps of every coordinate of `s` (all inside [0, n - 1])"""
    f = np.floor(s)
    u = s - f
    w = np.stack([(1 - u) ** 3 / 6, (3 * u ** 3 - 6 * u ** 2 + 4) / 6, (-3 * u ** 3 + 3 * u ** 2 + 3 * u + 1) / 6, u ** 3 / 6])
    q = f.astype(np.int64)[None, :] + np.arange(-1, 3)[:, None]
    return _mirror(q, n), w


def source_coords(warp: Warp, shape):
    """-> (sy, sx float64 [ho, wo], inside bool [ho, wo]) for a source of `shape`: off + m0 oy + m1 ox, added in that order"""
    ho, wo = warp.out_shape
    oy, ox = np.arange(ho, dtype=np.float64)[:, None], np.arange(wo, dtype=np.float64)[None, :]
    m, off = warp.matrix, warp.offset
    sy = (off[0] + m[0, 0] * oy) + m[0, 1] * ox
    sx = (off[1] + m[1, 0] * oy) + m[1, 1] * ox
    h, w = shape
    inside = (sy >= 0) & (sy <= h - 1) & (sx >= 0) & (sx <= w - 1)
    return sy, sx, inside


def plane_values(canvas: np.ndarray, warp: Warp, values: Sequence[int]) -> np.ndarray:
    """float64 [ho, wo, len(values)]: 255 S_c, the grey level before rounding, of the warped plane [canvas == c] for every c of
    `values`; 0 where the source coordinate lies outside the canvas."""
    canvas = np.asarray(canvas)
    h, w = canvas.shape
    ho, wo = warp.out_shape
    out = np.zeros((ho, wo, len(values)), dtype=np.float64)
    sy, sx, inside = source_coords(warp, (h, w))
    if not inside.any() or len(values) == 0:
        return out
    qy, wy = _taps(sy[inside], h)
    qx, wx = _taps(sx[inside], w)
    ay, ax = _prefilter(h), _prefilter(w)
    for k, c in enumerate(values):
        plane = canvas == c
        if not plane.any():
            continue
        coef = ay @ plane.astype(np.float64) @ ax.T
        acc = np.zeros(qy.shape[1], dtype=np.float64)
        for a in range(4):
            row = np.zeros_like(acc)
            for b in range(4):
                row += wx[b] * coef[qy[a], qx[b]]               # (a window gather per output pixel)
            acc += wy[a] * row
        out[..., k][inside] = 255.0 * acc
    return out


def _label_of(set_planes: np.ndarray) -> np.ndarray:
    """the generator's one-hot consistency loop on thresholded planes [..., n_class] (plane 0 plays no part): 1 if plane 1 is set,
    else the smallest set plane >= 2, else 0"""
    n_class = set_planes.shape[-1]
    lab = np.zeros(set_planes.shape[:-1], dtype=np.int64)
    for c in range(n_class - 1, 1, -1):
        lab[set_planes[..., c]] = c
    if n_class > 1:
        lab[set_planes[..., 1]] = 1
    return lab


def warp_host(ids, labels, aux, warp: Warp, n_token: int, n_class: int):
    """One document: ids / labels / aux integer [h, w] (ids in [0, n_token), labels in [0, n_class)) -> (multi-hot uint8
    [ho, wo, n_token], labels int64 [ho, wo], aux int64 [ho, wo]) as the generator's warp leaves them."""
    ids, labels, aux = np.asarray(ids), np.asarray(labels), np.asarray(aux)
    ho, wo = warp.out_shape
    hot = np.zeros((ho, wo, n_token), dtype=np.uint8)
    present = [int(c) for c in np.unique(ids) if 0 <= c < n_token]
    hot[..., present] = plane_values(ids, warp, present) > THRESHOLD
    outs = []
    for canvas in (labels, aux):
        planes = np.zeros((ho, wo, n_class), dtype=bool)
        present = [int(c) for c in np.unique(canvas) if 1 <= c < n_class]
        planes[..., present] = plane_values(canvas, warp, present) > THRESHOLD
        outs.append(_label_of(planes))
    return hot, outs[0], outs[1]


# ---- the launch ---------------------------------------------------------------------------------------------------------------------
def warped_canvas(warps: Sequence, round_to: int = 16):
    """-> (sizes int64 [B, 2] of the warped documents, (Ho, Wo) of their canvas: the largest of each, rounded up to `round_to`)"""
    sizes = np.array([w.out_shape for w in warps], dtype=np.int64).reshape(len(warps), 2)
    Ho, Wo = (int(-(-max(int(sizes[:, d].max()), 1) // round_to) * round_to) for d in (0, 1))
    return sizes, (Ho, Wo)


def warp_train_device(ids, labels, aux, sizes, warps: Sequence[Warp], grid, n_token: int, n_class: int, dtype: int):
    """The painter's canvases (ids int32, labels / aux int64 [B, H, W] on the device, sizes CPU [B, 2]) warped into `grid`, the
    NHWC input [B, Ho, Wo, Cs] in the storage dtype (`dtype`: _lib.F32 / BF16), by one launch of `msau_kv_warp_train` on the
    current stream -> (labels int64, aux int64 [B, Ho, Wo] on the device, flags int32 [B] on the device).  Every element of the
    three outputs is written by the launch: channels all zero, labels -1 outside a document's warped extent.  A document whose flag
    is not 0 has to be warped on the host (`warp_host`); `TrainEngine.step_kv` does that."""
    import torch
    from .. import _lib as L
    B, H, W = ids.shape
    _, Ho, Wo, Cs = grid.shape
    assert len(warps) == B and grid.shape[0] == B and grid.is_contiguous() and ids.is_contiguous()
    dev = ids.device
    rec = np.stack([w.record() for w in warps])                                            # float64 [B, 6]
    dsz = np.array([w.out_shape for w in warps], dtype=np.int32).reshape(B, 2)
    ssz = np.ascontiguousarray(np.asarray(sizes), dtype=np.int32).reshape(B, 2)
    # one upload: the doubles first (8-byte aligned), then the two size tables
    blob = np.concatenate([rec.reshape(-1).view(np.uint8), ssz.reshape(-1).view(np.uint8), dsz.reshape(-1).view(np.uint8)])
    blob_d = torch.from_numpy(blob).to(dev)
    base = blob_d.data_ptr()
    labels_out = torch.empty((B, Ho, Wo), dtype=torch.int64, device=dev)
    aux_out = torch.empty((B, Ho, Wo), dtype=torch.int64, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = torch.empty((int(L.load().msau_kv_warp_train_ws_ints(B, Ho, Wo)),), dtype=torch.int32, device=dev)
    L.call("msau_kv_warp_train", torch.cuda.current_stream(dev).cuda_stream, dtype, ids.data_ptr(), labels.data_ptr(), aux.data_ptr(),
           base + 48 * B, base, base + 56 * B, B, H, W, Ho, Wo, n_token, Cs, n_class, grid.data_ptr(), labels_out.data_ptr(),
           aux_out.data_ptr(), flags.data_ptr(), ws.data_ptr())
    return labels_out, aux_out, flags


def upload_host_warp(b: int, table, warp: Warp, grid, labels_out, aux_out, n_token: int, n_class: int):
    """document `b` of a warped group, warped on the host and uploaded into its slices (the fallback for a flagged document)"""
    import torch
    from . import kv_data
    ids, lab, aux = kv_data.paint_train_host(table) if table.ok else kv_data.paint_train_painter(table)
    hot, wl, wa = warp_host(ids, lab, aux, warp, n_token, n_class)
    ho, wo = warp.out_shape
    _, Ho, Wo, Cs = grid.shape
    full = np.zeros((Ho, Wo, Cs), dtype=np.float32)
    full[:ho, :wo, :n_token] = hot
    grid[b].copy_(torch.from_numpy(full).to(grid.dtype))
    for dst, src in ((labels_out, wl), (aux_out, wa)):
        canvas = np.full((Ho, Wo), -1, dtype=np.int64)
        canvas[:ho, :wo] = src
        dst[b].copy_(torch.from_numpy(canvas))


# ---- the elastic warp ---------------------------------------------------------------------------------------------------------------
# `image_util.elastic_transform` draws two coarse random fields (one value per 25 x 25 pixels), smooths them, blows them up to the
# document with `scipy.misc.imresize(..., interp='bicubic')` -- by that removed function's source `bytescale` to uint8 and Pillow's
# bicubic resize, so a field is a uint8 [h, w] array, never negative -- and resamples every one-hot plane x 255 with
# `map_coordinates(order=1)` (mode "constant", cval 0) at
#
#     sy = oy + fy[oy, ox] * alpha_y,   sx = ox + fx[oy, ox] * alpha_x        float64: the product rounded, then the sum
#
# Outside [0, h-1] x [0, w-1] a plane is 0; inside it is bilinear on floor(s) and floor(s) + 1 (clamped to n - 1, where its weight
# is 0).  With uy = sy - floor(sy), ux = sx - floor(sx) and p = 255 [canvas(tap) == c] the grey level of plane c is, in this order,
#
#     (1 - uy) * ((1 - ux) * p00 + ux * p01) + uy * ((1 - ux) * p10 + ux * p11)
#
# scipy rounds a uint8 output as t + 0.5, truncated, and the generator keeps > 64: the plane is set iff its grey level >= 64.5
# (ELASTIC_THRESHOLD; scipy sums the four terms in another order, so a grey level within ~1e-13 of 64.5 is not pinned and no test
# rests on one).  A set plane needs S_c >= 0.2529 of the four weights, which sum to 1: at most three planes of a pixel are set.
ELASTIC_THRESHOLD = 64.5            # set iff the grey level >= this
ELASTIC_GRID = 25                   # pixels per cell of the generator's coarse field


@dataclass
class Elastic:
    """output pixel (oy, ox) reads the source at (oy + field_y[oy, ox] * alpha_y, ox + field_x[oy, ox] * alpha_x)"""
    field_y: np.ndarray                 # uint8 [h, w]
    field_x: np.ndarray                 # uint8 [h, w]
    alpha_y: float
    alpha_x: float
    out_shape: Tuple[int, int]          # (h, w): the output has the input's shape

    def __post_init__(self):
        self.out_shape = (int(self.out_shape[0]), int(self.out_shape[1]))
        for name in ("field_y", "field_x"):
            f = np.asarray(getattr(self, name))
            if f.dtype != np.uint8 or f.shape != self.out_shape:
                raise ValueError(f"Elastic: {name} must be uint8 {self.out_shape}, got {f.dtype} {f.shape}")
            setattr(self, name, np.ascontiguousarray(f))
        self.alpha_y, self.alpha_x = float(self.alpha_y), float(self.alpha_x)
        if not (np.isfinite(self.alpha_y) and np.isfinite(self.alpha_x)):
            raise ValueError(f"Elastic: alphas must be finite, got ({self.alpha_y}, {self.alpha_x})")


def identity_elastic(shape) -> Elastic:
    shape = (int(shape[0]), int(shape[1]))
    return Elastic(np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8), 0.0, 0.0, shape)


def bytescale(field: np.ndarray) -> np.ndarray:
    """`scipy.misc.bytescale(data)` (removed from scipy) with its defaults: the field's own range mapped onto 0 .. 255"""
    field = np.asarray(field, dtype=np.float64)
    cmin, cmax = field.min(), field.max()
    cscale = cmax - cmin
    if cscale == 0:
        cscale = 1
    return (((field - cmin) * (255.0 / cscale)).clip(0, 255) + 0.5).astype(np.uint8)


def imresize_bicubic(field: np.ndarray, shape) -> np.ndarray:
    """`scipy.misc.imresize(field, shape, interp='bicubic')` (removed from scipy) restated: `bytescale`, then Pillow's bicubic resize
    of the 8-bit image -> uint8 [shape].  The only function of the package that needs Pillow."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("kv_warp.imresize_bicubic: the generator's elastic warp resizes its fields with Pillow (through the removed "
                          "scipy.misc.imresize); install Pillow to draw elastic fields") from e
    data = bytescale(field)
    im = Image.frombytes("L", (data.shape[1], data.shape[0]), data.tobytes())
    resample = getattr(getattr(Image, "Resampling", Image), "BICUBIC")
    out = np.asarray(im.resize((int(shape[1]), int(shape[0])), resample=resample), dtype=np.uint8)
    return np.ascontiguousarray(out)


def elastic_field(shape, value_x: float, value_y: float, rs: np.random.RandomState) -> Elastic:
    """`image_util.elastic_transform`'s random fields for a document of `shape`: dx, then dy, from `rs` (the generator's own
    `RandomState(None)` cannot be seeded) on a grid of one value per 25 x 25 pixels, smoothed with sigma = 0.0025 min(shape) and
    resized to the document as uint8.  A document under 25 pixels on a side has an empty grid, on which the generator itself fails:
    ValueError."""
    from scipy.ndimage import gaussian_filter
    h, w = int(shape[0]), int(shape[1])
    ny, nx = h // ELASTIC_GRID, w // ELASTIC_GRID
    if ny < 1 or nx < 1:
        raise ValueError(f"elastic_field: a document of {h} x {w} has no {ELASTIC_GRID}-pixel cell (the generator fails on it too)")
    sigma = min(w, h) * 0.0025
    alpha_x, alpha_y = value_x * min(h, w), value_y * min(h, w)
    dx = gaussian_filter(rs.rand(ny, nx) * 2 - 1, sigma)
    dy = gaussian_filter(rs.rand(ny, nx) * 2 - 1, sigma)
    return Elastic(imresize_bicubic(dy, (h, w)), imresize_bicubic(dx, (h, w)), alpha_y, alpha_x, (h, w))


def elastic_coords(el: Elastic):
    """-> (sy, sx float64 [h, w]): oy + field_y * alpha_y and ox + field_x * alpha_x, the product rounded, then the sum"""
    h, w = el.out_shape
    oy, ox = np.arange(h, dtype=np.float64)[:, None], np.arange(w, dtype=np.float64)[None, :]
    return oy + el.field_y.astype(np.float64) * el.alpha_y, ox + el.field_x.astype(np.float64) * el.alpha_x


def elastic_values(canvas: np.ndarray, el: Elastic, values: Sequence[int]) -> np.ndarray:
    """float64 [h, w, len(values)]: the grey level before rounding (255 S_c) of the elastically warped plane [canvas == c] for every c
    of `values`, summed as (1 - uy) * ((1 - ux) * p00 + ux * p01) + uy * ((1 - ux) * p10 + ux * p11); 0 where the source coordinate
    lies outside the canvas."""
    canvas = np.asarray(canvas)
    h, w = canvas.shape
    if (h, w) != el.out_shape:
        raise ValueError(f"elastic_values: a canvas of {(h, w)} under fields of {el.out_shape}")
    out = np.zeros((h, w, len(values)), dtype=np.float64)
    sy, sx = elastic_coords(el)
    inside = (sy >= 0) & (sy <= h - 1) & (sx >= 0) & (sx <= w - 1)
    if not inside.any() or len(values) == 0:
        return out
    sy, sx = sy[inside], sx[inside]
    fy, fx = np.floor(sy), np.floor(sx)
    uy, ux = sy - fy, sx - fx
    vy, vx = 1.0 - uy, 1.0 - ux
    j0, i0 = fy.astype(np.int64), fx.astype(np.int64)
    j1, i1 = np.minimum(j0 + 1, h - 1), np.minimum(i0 + 1, w - 1)          # (clamped: its weight is then 0)
    t00, t01, t10, t11 = canvas[j0, i0], canvas[j0, i1], canvas[j1, i0], canvas[j1, i1]
    for k, c in enumerate(values):
        p00, p01, p10, p11 = (np.where(t == c, 255.0, 0.0) for t in (t00, t01, t10, t11))
        out[..., k][inside] = vy * (vx * p00 + ux * p01) + uy * (vx * p10 + ux * p11)
    return out


def elastic_host(ids, labels, aux, el: Elastic, n_token: int, n_class: int):
    """`warp_host` for the elastic warp: one document's ids / labels / aux [h, w] -> (multi-hot uint8 [h, w, n_token], labels int64
    [h, w], aux int64 [h, w]) as the generator's `elastic_transform`, threshold and consistency loop leave them."""
    ids, labels, aux = np.asarray(ids), np.asarray(labels), np.asarray(aux)
    h, w = el.out_shape
    hot = np.zeros((h, w, n_token), dtype=np.uint8)
    present = [int(c) for c in np.unique(ids) if 0 <= c < n_token]
    hot[..., present] = elastic_values(ids, el, present) >= ELASTIC_THRESHOLD
    outs = []
    for canvas in (labels, aux):
        planes = np.zeros((h, w, n_class), dtype=bool)
        present = [int(c) for c in np.unique(canvas) if 1 <= c < n_class]
        planes[..., present] = elastic_values(canvas, el, present) >= ELASTIC_THRESHOLD
        outs.append(_label_of(planes))
    return hot, outs[0], outs[1]


def elastic_records(warps: Sequence[Elastic], sizes, H: int, W: int):
    """-> (fields uint8 [B, H, W, 2] = (fy, fx) on the source canvas, zero outside the documents; alphas float64 [B, 2] = (alpha_y,
    alpha_x)): what `msau_kv_elastic_train` takes for documents of `sizes` [B, 2]"""
    B = len(warps)
    sizes = np.asarray(sizes).reshape(B, 2)
    alphas = np.zeros((B, 2), dtype=np.float64)
    fields = np.zeros((B, H, W, 2), dtype=np.uint8)
    for b, el in enumerate(warps):
        h, w = el.out_shape
        if (h, w) != (int(sizes[b, 0]), int(sizes[b, 1])) or h > H or w > W:
            raise ValueError(f"elastic_records: document {b} is {tuple(sizes[b])} on a canvas of {(H, W)}, its fields {el.out_shape}")
        alphas[b] = (el.alpha_y, el.alpha_x)
        fields[b, :h, :w, 0], fields[b, :h, :w, 1] = el.field_y, el.field_x
    return fields, alphas


def elastic_train_device(ids, labels, aux, sizes, warps: Sequence[Elastic], grid, n_token: int, n_class: int, dtype: int):
    """`warp_train_device` for a group of `Elastic`s: the painter's canvases [B, H, W] resampled into `grid` [B, Ho, Wo, Cs] by one
    launch of `msau_kv_elastic_train` -> (labels int64, aux int64 [B, Ho, Wo], flags int32 [B], all on the device).  A document's
    output extent is its source size.  One upload: the alphas, the sizes and the fields, (fy, fx) interleaved on the source canvas."""
    import torch
    from .. import _lib as L
    B, H, W = ids.shape
    _, Ho, Wo, Cs = grid.shape
    assert len(warps) == B and grid.shape[0] == B and grid.is_contiguous() and ids.is_contiguous()
    dev = ids.device
    ssz = np.ascontiguousarray(np.asarray(sizes), dtype=np.int32).reshape(B, 2)
    fields, alphas = elastic_records(warps, ssz, H, W)
    # one upload: the doubles first (8-byte aligned), then the size table, then the fields
    blob = np.concatenate([alphas.reshape(-1).view(np.uint8), ssz.reshape(-1).view(np.uint8), fields.reshape(-1)])
    blob_d = torch.from_numpy(blob).to(dev)
    base = blob_d.data_ptr()
    labels_out = torch.empty((B, Ho, Wo), dtype=torch.int64, device=dev)
    aux_out = torch.empty((B, Ho, Wo), dtype=torch.int64, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = torch.empty((int(L.load().msau_kv_elastic_train_ws_ints(B, Ho, Wo)),), dtype=torch.int32, device=dev)
    L.call("msau_kv_elastic_train", torch.cuda.current_stream(dev).cuda_stream, dtype, ids.data_ptr(), labels.data_ptr(), aux.data_ptr(),
           base + 16 * B, base + 24 * B, base, B, H, W, Ho, Wo, n_token, Cs, n_class, grid.data_ptr(), labels_out.data_ptr(),
           aux_out.data_ptr(), flags.data_ptr(), ws.data_ptr())
    return labels_out, aux_out, flags


def upload_host_elastic(b: int, table, el: Elastic, grid, labels_out, aux_out, n_token: int, n_class: int):
    """document `b` of an elastic group, warped on the host and uploaded into its slices (the fallback for a flagged document)"""
    import torch
    from . import kv_data
    ids, lab, aux = kv_data.paint_train_host(table) if table.ok else kv_data.paint_train_painter(table)
    hot, wl, wa = elastic_host(ids, lab, aux, el, n_token, n_class)
    ho, wo = el.out_shape
    _, Ho, Wo, Cs = grid.shape
    full = np.zeros((Ho, Wo, Cs), dtype=np.float32)
    full[:ho, :wo, :n_token] = hot
    grid[b].copy_(torch.from_numpy(full).to(grid.dtype))
    for dst, src in ((labels_out, wl), (aux_out, wa)):
        canvas = np.full((Ho, Wo), -1, dtype=np.int64)
        canvas[:ho, :wo] = src
        dst[b].copy_(torch.from_numpy(canvas))
