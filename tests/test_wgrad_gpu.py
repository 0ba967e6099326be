"""GPU: every instance msau_conv2d_wgrad can launch, msau_wgrad_reduce and msau_channel_sum against the float64 reference of
tests/wgrad_util.py, ELEMENT BY ELEMENT.  A case is one direct call on small tensors, run with integer inputs (the sum of the slabs
must equal the reference bit for bit) and with random ones (within 2e-5 of the sum of the magnitudes of the terms), at nslabs = 1, a
count that does not divide the tiles, and one tile each; the slab buffer starts as NaN with a guard band behind it, so a column an
idle workgroup did not clear, a tile that was skipped, a slice written at another row offset or a write past the last slab show up
at the element where they happen.  Every case asserts the family msau_wgrad_route names for it.  CASES is built without a device
(the route is host code): tests/test_wgrad_cpu.py checks that it reaches every instance the route can name.

What this found: the 64 -> 8 role-swapped kernel wrote the bias gradient (the "ones" column, k = 576) in chunk 0 only and 0 in the
chunks behind it (Cin = 128: got 0, want sum g, e.g. 48.32), where every other kernel and the slab layout of include/msau_hip.h
have it in every chunk.  msau_wgrad_reduce reads chunk 0, so no gradient was wrong; the kernel now writes it in every chunk.

653 tests, about 6 s on an MI355X.  Worst error / bound of the random runs per family (`pytest -s` prints them): generic 0.016,
lean 0.013, dilated / stride-2 0.016, 64 -> 8 0.003, id-fed 0.0002, row-streaming 0.002.
"""
import ctypes as C
import dataclasses

import pytest
import torch

from msau_amd import _lib as L
from tests import wgrad_util as U
from tests.wgrad_util import Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = L.F32, L.BF16
BOTH = (F32, BF16)
RELU, IDS = L.CONV_RELU_IN, L.CONV_IDS
ROWS4 = (("MSAU_WGRAD_ROWS4", "1"),)


# ---- the case table ----------------------------------------------------------------------------------------------------------
def _generic_representatives():
    """the cheapest descriptor of a small grid for every (dtype, CTN, NKW, compact, sliced) of the generic kernel the route names"""
    best = {}
    for c, rc, info in U.sweep((8, 16, 24, 40, 48, 64), (8, 24, 40, 72, 136), (1, 3, 4, 5, 7), (1, 16), (1, 2), hw=(19, 35), split=False):
        if rc == 0 and info[0] == U.GENERIC:
            key = U.route_tuple(c.dtype, info)
            cost = (c.k * c.k * c.C1 * c.Cout, c.name)
            if key not in best or cost < best[key][0]:
                best[key] = (cost, c)
    out = []
    for key in sorted(best):
        c = best[key][1]
        compact = key[4] == 1
        hw = (21, 40) if compact else c.hw
        hw_in = None if c.hw_in is None else (hw[0] + (c.k - 1) * c.dil, hw[1] + (c.k - 1) * c.dil)
        out.append(dataclasses.replace(c, name=f"ct{key[2]}nk{key[3]}{'c' if compact else ''}{'s' if key[5] else ''}-{c.name}", family=U.GENERIC,
                                       hw=hw, hw_in=hw_in, tup=key[2:]))
    return out


def _both(name, family, *a, dtypes=BOTH, **kw):
    fam = family if isinstance(family, dict) else {F32: family, BF16: family}
    return [Case(name, t, fam[t], *a, **kw) for t in dtypes]


def _cases():
    G, LN, SP = U.GENERIC, U.LEAN, U.SPECIAL
    cs = _generic_representatives()
    # ---- generic kernel: what the representatives leave out
    cs += _both("24to40-k3-relu", G, 24, 40, 3, flags=RELU)
    cs += _both("24+8to24-k3", G, 24, 24, 3, C2=8)                                   # cch forced below C1: 4 chunks of 8, the last from x2
    cs += _both("120to24-k3", G, 120, 24, 3)                                         # 3 chunks of 40
    cs += _both("192to24-k1", G, 192, 24, 1)                                         # 3 chunks of 64
    cs += _both("24to24-k3-s2", G, 24, 24, 3, stride=2)
    cs += _both("24to24-k3-s2-odd", G, 24, 24, 3, stride=2, hw_in=(37, 69))          # Hin = 2 Hout - 1
    cs += _both("8to56-k7", G, 8, 56, 7)
    cs += _both("16to128-k3", G, 16, 128, 3)
    cs += _both("48to24-k5-pad(1,3)", G, 48, 24, 5, pad=(1, 3))
    cs += _both("16to16-k3-valid", G, 16, 16, 3, pad=(0, 0), hw_in=(21, 37))         # a lean shape on the generic kernel: Hin != Hout
    cs += _both("32to32-k3-d2", G, 32, 32, 3, dil=2)
    # ---- compact form (dil >= 16: one 16 x 16 block per tap), 21 x 40
    for dil in (16, 32):
        cs += _both(f"16to40-k3-d{dil}", G, 16, 40, 3, dil=dil, hw=(21, 40))         # fp32: two slices of 32
        cs += _both(f"8+8to16-k3-d{dil}-relu", G, 8, 16, 3, C2=8, dil=dil, hw=(21, 40), flags=RELU)
    # ---- slices: the rows of every slice at their co0, the ones column in every chunk (3 chunks of 8, the last from x2)
    cs += [Case("16+8to136-k3", BF16, G, 16, 136, 3, C2=8), Case("16+8to256-k3", BF16, G, 16, 256, 3, C2=8, hw=(21, 40)),
           Case("16+8to72-k3", F32, G, 16, 72, 3, C2=8), Case("16+8to136-k3", F32, G, 16, 136, 3, C2=8)]
    # ---- lean: the eleven (cch / 8, Cout / 8) shapes at 1x1 and 3x3, 8 -> 8 at 4x4
    for c8, co8 in ((1, 1), (1, 2), (2, 1), (2, 2), (2, 4), (4, 2), (4, 4), (8, 1), (4, 8), (8, 4), (8, 8)):
        for k in (1, 3):
            fam = {F32: LN, BF16: U.IN64 if (c8, co8, k) == (8, 1, 3) else LN}
            cs += _both(f"{8 * c8}to{8 * co8}-k{k}", fam, 8 * c8, 8 * co8, k)
    cs += _both("8to8-k4", LN, 8, 8, 4)
    for pad in ((0, 0), (2, 2), (2, 0), (0, 1)):
        cs += _both(f"16to16-k3-pad{pad}", LN, 16, 16, 3, pad=pad)
        cs += _both(f"32to64-k3-pad{pad}", LN, 32, 64, 3, pad=pad)
    for pad in ((0, 0), (3, 3), (1, 2)):
        cs += _both(f"8to8-k4-pad{pad}", LN, 8, 8, 4, pad=pad)
    for k in (1, 3):
        cs += _both(f"8+8to16-k{k}", LN, 8, 16, k, C2=8)
        cs += _both(f"16+16to16-k{k}", LN, 16, 16, k, C2=16)
    cs += _both("32to32-k3-relu", LN, 32, 32, 3, flags=RELU)
    cs += _both("8+8to8-k1-relu", LN, 8, 8, 1, C2=8, flags=RELU)
    # ---- the six dilated / stride-2 instances (fp32 stages 32 channels of this halo in chunks of 16: the generic kernel takes it)
    for cin, dil in ((8, 2), (16, 4), (32, 8)):
        fam = {F32: G if cin == 32 else SP, BF16: SP}
        cs += _both(f"{cin}to{2 * cin}-k3-d{dil}", fam, cin, 2 * cin, 3, dil=dil)
        cs += _both(f"{cin}to{2 * cin}-k3-s2", fam, cin, 2 * cin, 3, stride=2)
    cs += [Case("16to32-k3-s2-odd", BF16, SP, 16, 32, 3, stride=2, hw_in=(37, 69))]
    # ---- the 64 -> 8 role-swapped instance (bf16), one and two chunks, every pad it takes; fed with ids
    for cin in (64, 128):
        for pad in ((0, 0), (1, 1), (2, 2), (0, 2), (2, 1)):
            cs += [Case(f"{cin}to8-k3-pad{pad}", BF16, U.IN64, cin, 8, 3, pad=pad)]
    cs += [Case("32+32to8-k3", F32, G, 32, 8, 3, C2=32), Case("64+64to8-k3-relu", BF16, U.IN64, 64, 8, 3, C2=64, flags=RELU)]
    for pad in ((1, 1), (0, 2)):
        cs += [Case(f"ids64to8-k3-pad{pad}", BF16, U.IN64_IDS, 64, 8, 3, pad=pad, flags=IDS)]
    # ---- the row-streaming instance (bf16 8 -> 8, 3x3 and under MSAU_WGRAD_ROWS4 4x4): 2 * 3 * 5 = 30 tasks, the threshold is 16
    rows = dict(hw=(33, 61), nslabs=(1, 5, 24))
    cs += [Case("8to8-k3-rows", BF16, U.ROWS, 8, 8, 3, **rows), Case("8to8-k3-rows-relu", BF16, U.ROWS, 8, 8, 3, flags=RELU, **rows),
           Case("8to8-k3-15tasks", BF16, LN, 8, 8, 3, B=1, hw=(33, 61)),                           # just below MSAU_ROWS_MIN_TASKS
           Case("8to8-k4-rows4", BF16, U.ROWS, 8, 8, 4, env=ROWS4, **rows), Case("8to8-k4-rows4-relu", BF16, U.ROWS, 8, 8, 4, flags=RELU, env=ROWS4, **rows),
           Case("8to8-k4-rows4-off", BF16, LN, 8, 8, 4, **rows),
           Case("8to8-k3-rows-32slabs-16tasks", BF16, U.ROWS, 8, 8, 3, B=8, hw=(18, 30), nslabs=(32,))]   # more workgroups than tasks
    # ---- the edge geometries, once per family and type: one full tile, one row, one column, three samples on four workgroups
    reps = {(U.GENERIC, F32): ("24to40-k3", 24, 40, {}), (U.GENERIC, BF16): ("24to40-k3", 24, 40, {}),
            (U.LEAN, F32): ("16to32-k3", 16, 32, {}), (U.LEAN, BF16): ("16to32-k3", 16, 32, {}),
            (U.SPECIAL, F32): ("8to16-k3-s2", 8, 16, dict(stride=2)), (U.SPECIAL, BF16): ("16to32-k3-d4", 16, 32, dict(dil=4)),
            (U.IN64, BF16): ("128to8-k3", 128, 8, {}), (U.IN64_IDS, BF16): ("ids64to8-k3", 64, 8, dict(flags=IDS)),
            (U.ROWS, BF16): ("8to8-k3", 8, 8, {})}
    for (fam, t), (name, cin, cout, kw) in reps.items():
        for hw, B, ns in (((16, 16), 2, (1, 2)), ((1, 40), 2, (1, 4, 6)), ((33, 1), 2, (1, 4, 6)), ((19, 35), 3, (4,))):
            if fam == U.ROWS:                         # enough samples for MSAU_ROWS_MIN_TASKS tasks of 8 rows x 30 columns
                B = {(16, 16): 8, (1, 40): 8, (33, 1): 4}.get(hw, B)
                hw = (33, 61) if B == 3 else hw
                ns = (1, B) if B > 3 else ns
            cs.append(Case(f"{name}-{hw[0]}x{hw[1]}-B{B}", t, fam, cin, cout, 3, B=B, hw=hw, nslabs=ns, **kw))
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return cs


CASES = _cases()
# grouped launches (msau_conv2d_wgrad_group): one lean and one special shape
GROUPED = [Case("16to16-k3", t, U.LEAN, 16, 16, 3) for t in BOTH] + [Case("8to16-k3-d2", t, U.SPECIAL, 8, 16, 3, dil=2) for t in BOTH]
WORST = {}


@pytest.fixture
def wenv(monkeypatch):
    """MSAU_* switches for one test: set, have the library read them again, and the same on the way out"""
    lib = L.load()

    names = set()

    def set_env(pairs):
        for k in names:
            monkeypatch.delenv(k, raising=False)
        for k, v in pairs:
            monkeypatch.setenv(k, v)
            names.add(k)
        lib.msau_reload_env()
    yield set_env
    monkeypatch.undo()
    lib.msau_reload_env()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam, r in sorted(WORST.items()):
        print(f"\nworst err/bound, random inputs, {U.FAMILY[fam]:9s} {r:.3g}")


def _on_device(c, kind, seed=0):
    ins = {k: (v.to(DEV) if v is not None else None) for k, v in U.make_inputs(c, kind, seed).items()}
    xt, g = U.x_tilde(c, ins["x1"], ins["x2"]), ins["g"].double()
    return ins, xt, g


def _expect(c, xt, g, info):
    ref, mask = U.reference(c, xt, g, info[5], info[6], info[7])
    S, _ = U.reference(c, xt.abs(), g.abs(), info[5], info[6], info[7])
    return ref, S, mask


def _launch(c, ins, nslabs, info):
    buf = U.slab_buffer(nslabs, info[6] * c.Cout * info[7], DEV)
    d = U.descriptor(c, nslabs, ins["x1"].data_ptr(), ins["x2"].data_ptr() if ins["x2"] is not None else None, ins["g"].data_ptr(), buf.data_ptr())
    L.call("msau_conv2d_wgrad", torch.cuda.current_stream().cuda_stream, c.dtype, C.byref(d))
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("kind", ["int", "rand"])
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_wgrad_instance(c, kind, wenv):
    wenv(c.env)
    rc, info = U.route(c.dtype, U.descriptor(c))
    assert rc == 0 and info[0] == c.family, f"written for the {U.FAMILY[c.family]} family, the route says {info} (status {rc})"
    assert c.tup is None or (info[1], info[2], info[3], int(info[4] > 1)) == c.tup, (info, c.tup)
    ins, xt, g = _on_device(c, kind)
    ref, S, mask = _expect(c, xt, g, info)
    for nslabs in c.nslabs:
        assert nslabs <= c.ntiles
        buf = _launch(c, ins, nslabs, info)
        r = U.check_slabs(buf, nslabs, ref, S, mask, kind, f"{c.id} nslabs {nslabs} {kind}")
        if kind == "rand":
            WORST[c.family] = max(WORST.get(c.family, 0.0), r)


@pytest.mark.parametrize("pad", [(1, 1), (0, 2), (2, 0)])
def test_id_fed_launch_writes_the_bits_of_the_dense_one(pad):
    """include/msau_hip.h: the one-hot tile synthesised from the ids is bit-identical to the dense launch of the same page"""
    ci = Case("ids", BF16, U.IN64_IDS, 64, 8, 3, pad=pad, flags=IDS)
    cd = dataclasses.replace(ci, family=U.IN64, flags=0)
    ins, _, _ = _on_device(ci, "rand")
    dense = dict(ins, x1=U.onehot(ins["x1"]).to(torch.bfloat16).contiguous())
    for c in (ci, cd):
        assert U.route(BF16, U.descriptor(c))[1][0] == c.family
    info = U.route(BF16, U.descriptor(ci))[1]
    for nslabs in (1, 5, 12):
        a, b = _launch(ci, ins, nslabs, info), _launch(cd, dense, nslabs, info)
        n = nslabs * 8 * info[7]
        assert torch.equal(a[:n].view(torch.int32), b[:n].view(torch.int32))
        assert bool(torch.isfinite(a[:n].view(nslabs, 8, info[7])[..., :577]).all())


@pytest.mark.parametrize("kind", ["int", "rand"])
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("c", GROUPED, ids=[c.id for c in GROUPED])
def test_grouped_launch_against_the_reference(c, n, kind):
    """msau_conv2d_wgrad_group: n launches of one shape in one grid, each layer's slabs against ITS reference (n = 3: the one padded
    slot of the argument struct is neither empty nor absent)"""
    lib = L.load()
    rc, info = U.route(c.dtype, U.descriptor(c))
    assert rc == 0 and info[0] == c.family
    nslabs = 5
    layers, descs = [], []
    for i in range(n):
        ins, xt, g = _on_device(c, kind, seed=i + 1)
        buf = U.slab_buffer(nslabs, info[6] * c.Cout * info[7], DEV)
        layers.append((ins, _expect(c, xt, g, info), buf))
        descs.append(U.descriptor(c, nslabs, ins["x1"].data_ptr(), None, ins["g"].data_ptr(), buf.data_ptr()))
    assert lib.msau_conv2d_wgrad_groupable(c.dtype, C.byref(descs[0]), C.byref(descs[-1])) == 1
    arr = (C.POINTER(L.WgradDesc) * n)(*[C.pointer(d) for d in descs])
    L.check(lib.msau_conv2d_wgrad_group(torch.cuda.current_stream().cuda_stream, c.dtype, arr, n), "wgrad_group")
    torch.cuda.synchronize()
    for i, (_, (ref, S, mask), buf) in enumerate(layers):
        U.check_slabs(buf, nslabs, ref, S, mask, kind, f"{c.id} group of {n}, layer {i}, {kind}")


# ---- msau_channel_sum ----------------------------------------------------------------------------------------------------------
# channel_sum_kernel: 256 threads, thread t owns channel group t % (Cs / 8) of the pixels blk * ppb + t / (Cs / 8) + i * nblk * ppb,
# ppb = 256 / (Cs / 8); four loads in flight while p + 3 * nblk * ppb < npix.  Edges: one block; blocks that do not divide the pixels;
# more blocks than npix / 256 (whole blocks idle: they must write zeros); fewer pixels than one block's rows; the 4-deep loop entered
# and not; Cs from one channel group (ppb 256) to 32 (ppb 8).
CSUM = [(8, 1, 1), (8, 255, 1), (8, 1031, 1), (8, 1031, 3), (8, 5000, 2), (8, 700, 5), (16, 515, 3), (16, 4099, 2), (32, 333, 7), (64, 257, 4),
        (128, 100, 3), (256, 77, 2), (256, 2051, 16), (8, 2 * 19 * 35, 256)]


@pytest.mark.parametrize("kind", ["int", "rand"])
@pytest.mark.parametrize("dtype", BOTH, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cs,npix,nblk", CSUM)
def test_channel_sum(Cs, npix, nblk, dtype, kind):
    gen = torch.Generator().manual_seed(3)
    g = U.draw(kind, (npix, Cs), gen, dtype).to(DEV)
    buf = torch.full((nblk * Cs + U.GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    L.call("msau_channel_sum", torch.cuda.current_stream().cuda_stream, dtype, g.data_ptr(), npix, Cs, buf.data_ptr(), nblk)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[nblk * Cs:]).all()), "written behind the partials"
    part = buf[:nblk * Cs].view(nblk, Cs)
    assert bool(torch.isfinite(part).all()), "a block left its row of partials unwritten"
    got, want, mag = part.double().sum(0), g.double().sum(0), g.double().abs().sum(0)
    if kind == "int":
        assert float(mag.max()) < 2 ** 24 and torch.equal(got, want)
    else:
        # the worst case of an fp32 sum of npix terms in any order (the block partials are summed here in float64)
        assert bool(((got - want).abs() <= npix * 2.0 ** -24 * mag).all()), float(((got - want).abs() / mag).max())


# ---- msau_wgrad_reduce: hand-built tables over synthetic slabs ---------------------------------------------------------------------
SENT = -7.5e4                      # between and around the parameters of the flat gradient buffer
PREFILL = 3.0                      # what accumulate = 1 adds to (exact in the integer runs)


def _entry(kind, nslabs, b_nslabs, accumulate):
    """(fields of an msau_unpack_entry without offsets, O, I) -- OIHW weight [O][I][k][k] of a conv, IOHW [O = dim0][I][k][k] of a transposed one"""
    e = dict(nslabs=nslabs, accumulate=accumulate, row_is_dim0=1, k2_real=0, k2_store=0)
    if kind == "conv1":                         # one chunk, every row and channel real
        e.update(KH=3, KW=3, cch=16, nchunks=1, rows_store=8, rows_real=8, k1_real=16, k1_store=16, bias="ones")
    elif kind == "conv2":                       # two chunks, a padded first source and padded rows: 5 of 8 | 8, 6 of 8 rows
        e.update(KH=3, KW=3, cch=8, nchunks=2, rows_store=8, rows_real=6, k1_real=5, k1_store=8, k2_real=8, k2_store=8, bias="ones")
    elif kind == "conv1x1":                     # 1x1, three chunks, padded second source, more rows than one 64-float run
        e.update(KH=1, KW=1, cch=8, nchunks=3, rows_store=24, rows_real=21, k1_real=16, k1_store=16, k2_real=3, k2_store=8, bias="ones")
    elif kind == "deconv":                      # transposed conv: rows = its input channels, bias from channel-sum partials
        e.update(KH=3, KW=3, cch=16, nchunks=1, rows_store=8, rows_real=7, k1_real=13, k1_store=16, bias="csum", b_nslabs=b_nslabs, b_count=13)
    elif kind == "nobias":
        e.update(KH=4, KW=4, cch=8, nchunks=1, rows_store=8, rows_real=8, k1_real=8, k1_store=8, bias=None)
    e["kext"] = -(-(e["KH"] * e["KW"] * e["cch"] + 8) // 16) * 16
    e["dim0"], e["dim1"] = e["rows_real"], e["k1_real"] + e["k2_real"]
    return e


def _reduce_case(entries, kind, seed=0):
    """arena, flat buffer, table and the float64 expectation (values, bounds) for a list of _entry()s"""
    gen = torch.Generator().manual_seed(50 + seed)
    arena, flat_n, recs = [], 64, []
    off = 0

    def values(shape):
        return U.draw(kind, shape, gen, L.F32)
    for e in entries:
        taps, cch, kext, nch, rs = e["KH"] * e["KW"], e["cch"], e["kext"], e["nchunks"], e["rows_store"]
        slab = values((e["nslabs"], nch, rs, kext))
        real = torch.zeros(nch, rs, kext, dtype=torch.bool)               # positions the entry must read; everything else is NaN
        chan = torch.full((nch * cch,), -1, dtype=torch.long)             # stored channel -> real channel of the parameter
        for cs in range(nch * cch):
            if cs < e["k1_store"]:
                chan[cs] = cs if cs < e["k1_real"] else -1
            elif cs - e["k1_store"] < e["k2_real"]:
                chan[cs] = e["k1_real"] + cs - e["k1_store"]
        for ch in range(nch):
            for c in range(cch):
                if chan[ch * cch + c] >= 0:
                    real[ch, :e["rows_real"], c:taps * cch:cch] = True
        if e["bias"] == "ones":
            real[0, :e["rows_real"], taps * cch] = True
        slab = torch.where(real[None], slab, torch.tensor(float("nan")))
        e["slab_off"], e["slab_elems"] = off, nch * rs * kext
        arena.append(slab.reshape(-1))
        off += slab.numel()
        pad = (-off) % 64                                                  # (slabs are 256-byte aligned: the kernel reads float4)
        arena.append(torch.full((pad,), float("nan")))
        off += pad
        tot, mag = slab.double().sum(0), slab.double().abs().sum(0)
        w = torch.zeros(e["dim0"], e["dim1"], e["KH"], e["KW"], dtype=torch.float64)
        wm = torch.zeros_like(w)
        for ch in range(nch):
            for c in range(cch):
                kc = int(chan[ch * cch + c])
                if kc >= 0:
                    w[:, kc] = tot[ch, :e["rows_real"], c:taps * cch:cch].reshape(e["dim0"], e["KH"], e["KW"])
                    wm[:, kc] = mag[ch, :e["rows_real"], c:taps * cch:cch].reshape(e["dim0"], e["KH"], e["KW"])
        e["w_off"] = flat_n
        flat_n += w.numel() + 37
        rec = {"e": e, "w": w, "wm": wm, "b": None}
        e["b_off"], e["b_src_off"], e["b_slab_stride"], e["b_elem_stride"] = -1, 0, 0, 0
        e.setdefault("b_nslabs", 0)
        e.setdefault("b_count", 0)
        if e["bias"] == "ones":
            e.update(b_src_off=e["slab_off"] + taps * cch, b_slab_stride=e["slab_elems"], b_elem_stride=kext, b_nslabs=e["nslabs"], b_count=e["rows_real"])
            rec["b"], rec["bm"] = tot[0, :e["rows_real"], taps * cch], mag[0, :e["rows_real"], taps * cch]
        elif e["bias"] == "csum":
            cs_store = 16                                                  # partials [b_nslabs][16], 13 real channels
            part = values((e["b_nslabs"], cs_store))
            part[:, e["b_count"]:] = float("nan")
            e.update(b_src_off=off, b_slab_stride=cs_store, b_elem_stride=1)
            arena.append(part.reshape(-1))
            off += part.numel()
            pad = (-off) % 64
            arena.append(torch.full((pad,), float("nan")))
            off += pad
            rec["b"], rec["bm"] = part[:, :e["b_count"]].double().sum(0), part[:, :e["b_count"]].double().abs().sum(0)
        if rec["b"] is not None:
            e["b_off"] = flat_n
            flat_n += rec["b"].numel() + 5
        recs.append(rec)
    table = (L.UnpackEntry * len(entries))()
    for t, e in zip(table, entries):
        for name, _ in L.UnpackEntry._fields_:
            setattr(t, name, e[name])
    return torch.cat(arena), flat_n + 64, recs, table


REDUCE = [("conv1", ns, 0) for ns in (1, 15, 16, 17, 63, 64, 65, 130)] + [("conv2", ns, 0) for ns in (1, 17, 65)] + \
         [("conv1x1", ns, 0) for ns in (16, 130)] + [("deconv", 5, bn) for bn in (1, 3, 16, 17, 256)] + [("deconv", 64, 17), ("nobias", 17, 0)]


def _run_reduce(entries, kind):
    arena, flat_n, recs, table = _reduce_case(entries, kind)
    flat = torch.full((flat_n,), SENT, dtype=torch.float32)
    touched = torch.zeros(flat_n, dtype=torch.bool)
    for r in recs:
        e = r["e"]
        spans = [(e["w_off"], r["w"].numel())] + ([(e["b_off"], r["b"].numel())] if r["b"] is not None else [])
        for o, n in spans:
            flat[o:o + n] = PREFILL
            touched[o:o + n] = True
    flat_d, arena_d = flat.to(DEV), arena.to(DEV)
    table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    L.call("msau_wgrad_reduce", torch.cuda.current_stream().cuda_stream, arena_d.data_ptr(), flat_d.data_ptr(), table_d.data_ptr(), len(entries),
           max(r["e"]["slab_elems"] for r in recs))
    torch.cuda.synchronize()
    out = flat_d.cpu()
    assert torch.equal(out[~touched], flat[~touched]), "the flat buffer was written between or around the parameters"
    assert bool(torch.isfinite(out).all()), "a slab position the entry must discard (NaN here) reached the gradient"
    for i, r in enumerate(recs):
        e = r["e"]
        for what, off, want, mag, ns in (("weight", e["w_off"], r["w"], r["wm"], e["nslabs"]),) + \
                ((("bias", e["b_off"], r["b"], r["bm"], e["b_nslabs"]),) if r["b"] is not None else ()):
            got = out[off:off + want.numel()].double().view(want.shape)
            want = want + (PREFILL if e["accumulate"] else 0.0)
            if kind == "int":
                assert float(mag.max()) + PREFILL < 2 ** 24
                assert torch.equal(got, want), f"entry {i} {what}: {int((got != want).sum())} elements differ"
            else:
                # fp32 sum of ns terms in any order, and one more rounding where the result is added to the gradient
                bound = ns * 2.0 ** -24 * mag + (2.0 ** -24 * (want.abs() + PREFILL) if e["accumulate"] else 0.0)
                assert bool(((got - want).abs() <= bound).all()), f"entry {i} {what}: {float(((got - want).abs() - bound).max()):.3g} over"


@pytest.mark.parametrize("kind", ["int", "rand"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("what,nslabs,b_nslabs", REDUCE)
def test_wgrad_reduce_one_entry(what, nslabs, b_nslabs, accumulate, kind):
    _run_reduce([_entry(what, nslabs, b_nslabs, accumulate)], kind)


@pytest.mark.parametrize("kind", ["int", "rand"])
def test_wgrad_reduce_several_entries(kind):
    """one call, five entries of different sizes (the grid is sized by the largest), overwriting and accumulating side by side"""
    _run_reduce([_entry("conv1", 17, 0, 0), _entry("deconv", 3, 17, 1), _entry("conv1x1", 64, 0, 1), _entry("conv2", 130, 0, 0),
                 _entry("nobias", 1, 0, 1), _entry("deconv", 65, 256, 0)], kind)
