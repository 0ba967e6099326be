"""The attention core's float64 reference, its per-element error bounds, the input generators of the attention tests and a
torch emulation of the kernels' roundings (tests/test_attention_cpu.py, tests/test_attention_gpu.py).

Formulae (csrc/attention.hip, csrc/attention_mfma.hip, oracle.msau_oracle.self_attention; rows of s are normalised, the output
sums over ROWS):
    s_ij = g_i . f_j        P = softmax_j(s)        y_j = x_j + sum_i P_ij h_i
    dh_i = sum_j P_ij dy_j  delta_i = h_i . dh_i    dS_ij = P_ij (h_i . dy_j - delta_i)
    dg_i = sum_j dS_ij f_j  df_j = sum_i dS_ij g_i
With an extent, sample b is its (h_b, w_b) crop of the W-wide grid evaluated alone: keys outside get P = 0, own positions outside
get y = x and dh = delta = dg = df = 0.

Bounds, per element (S: a sum of |terms|, returned by attn_ref beside every output):
    fp32 storage            |got - ref| <= ACC S
    bf16 storage, VALU      |got - ref| <= 1/2 ulp_bf16 + ACC S                 (fp32 arithmetic, one rounding at the store)
    bf16 storage, MFMA      |got - ref| <= 1/2 ulp_bf16 + 2^-8 S1 + K S2        (P and dS enter the second product as bf16)
  y, dh:   S = S1 = sum |P h| (+ |x|), sum |P dy|
  dg, df:  S1 = sum |dS f|, sum |dS g|;  S = S2 = sum_j P_ij (A_ij + sum_j' P_ij' A_ij') |f_jd| with A_ij = sum_c |h_ic| |dy_jc|:
           the cancellation in h . dy - delta is charged at the size of its operands
  delta:   S = sum_c |h_ic| sum_j P_ij |dy_jc|
  m:       ACC sum_d |g_id| |f_jd| at the arg-max;   ln Z and m + ln Z:  1e-5 + ACC max_j sum_d |g_id| |f_jd|
           (m + ln Z is what the sweeps consume: it inherits the score error, once, and the fp32 exp / log of the row sum)
ACC = 3e-5 is the project's fp32 accumulation slack (tests/test_launch_ulp_gpu.py).

Two constants of the MFMA family are NOT the fp32 slack, because the MFMA backward takes delta_i from the dh sweep's accumulators,
i.e. from probabilities already rounded to bf16 (relative error <= 2^-9 each, and on a nearly one-hot row it is ONE term: nothing
averages).  That error is a fraction of S(delta), and through P_ij delta_i of S2(dg), S2(df).  Both constants are calibrated
by one rule -- against float64 versus the emulation below (P and dS rounded to bf16 in torch, fp32 sums; never against the
kernel), over every generator at the sizes of the CPU test, and set to at most 2x the worst ratio measured there:
    K_DELTA_MFMA = 2^-9 + ACC   worst |delta_emulated - delta_ref| / S(delta) measured 1.91e-3 = 0.98 * 2^-9 (peaked generator;
                          1.1e-3 normal, 1.3e-3 / 1.5e-3 shifted): the analytic worst case, every probability of a row off by half
                          a bf16 ulp with one sign, plus the fp32 slack of the sum itself.  (With ACC alone: 64x too tight.)
    K_CANCEL_MFMA = 1.5e-3      worst (|d - ref| - 1/2 ulp - 2^-8 S1) / S2 over dg, df measured 8.0e-4 (peaked generator; 3.0e-4
                          normal, 2.6e-4 / 3.7e-4 shifted): the same error, passed on by P_ij delta_i.  1.9x the measured value.
                          (With ACC alone: 27x too tight.)
tests/test_attention_cpu.py repeats both measurements and holds the constants to the 2x rule.
Every other constant is the fp32 slack or the forward check's 2^-8 (tests/test_launch_ulp_gpu.py)."""
import torch

from tests.test_launch_ulp_gpu import ACC, assert_rounded, ulp_bf16

K_P_BF16 = 2.0 ** -8            # P / dS rounded to bf16 ahead of the second product: 2^-9 of every |term|, doubled (the forward check's constant)
K_DELTA_MFMA = 2.0 ** -9 + ACC  # see the module docstring (emulation: 1.91e-3)
K_CANCEL_MFMA = 1.5e-3          # see the module docstring (emulation: 8.0e-4)
LNZ_ABS = 1e-5

OUTPUTS = ("m", "lnZ", "lse", "y", "dh", "delta", "dg", "df")
GENERATORS = ("normal", "peaked", "shift_neg", "shift_pos", "f_zero", "h_zero")


def extent_mask(extent_b, N, W, device):
    """[N] bool: the positions of the W-wide grid inside (h, w)"""
    j = torch.arange(N, device=device)
    return (j // W < int(extent_b[0])) & (j % W < int(extent_b[1]))


def attn_ref(f, g, h, x, dy, extent=None, W=None, device=None):
    """f, g [B, N, D]; h, x, dy [B, N, C]: the values stored on the device (fp32, or bf16 cast up); extent [B, 2] = (h_b, w_b) on the
    W-wide grid or None.  -> dict of float64 tensors on `device`: m, Z, lnZ, lse [B, N]; y, dh [B, N, C]; delta [B, N]; dg, df
    [B, N, D]; and under "S" the sums of |terms| of the bounds.  One sample at a time: a handful of N x N matrices are alive."""
    device = torch.device(device) if device is not None else f.device
    B, N, D = f.shape
    out = {k: [] for k in ("m", "Z", "y", "dh", "delta", "dg", "df")}
    S = {k: [] for k in ("m", "sc", "y", "dh", "delta", "dg1", "dg2", "df1", "df2")}
    for b in range(B):
        fb, gb, hb, xb, dyb = (t[b].to(device=device, dtype=torch.float64) for t in (f, g, h, x, dy))
        inn = torch.ones(N, dtype=torch.bool, device=device) if extent is None else extent_mask(extent[b], N, W, device)
        s = gb @ fb.T
        s[:, ~inn] = -float("inf")
        m, jmax = s.max(1)
        A = gb.abs() @ fb.abs().T
        S["m"].append(A.gather(1, jmax[:, None])[:, 0])
        S["sc"].append(A[:, inn].max(1).values)
        del A
        P = torch.exp(s - m[:, None])
        del s
        Z = P.sum(1)
        P /= Z[:, None]
        P[~inn] = 0                                     # a row outside the extent is not part of the sample
        out["m"].append(m); out["Z"].append(Z)
        out["y"].append(xb + P.T @ hb)
        S["y"].append(P.T @ hb.abs())
        dh, Sdh = P @ dyb, P @ dyb.abs()
        delta, Sdelta = (hb * dh).sum(1), (hb.abs() * Sdh).sum(1)
        out["dh"].append(dh); S["dh"].append(Sdh); out["delta"].append(delta); S["delta"].append(Sdelta)
        dS = hb @ dyb.T
        dS -= delta[:, None]
        dS *= P
        out["dg"].append(dS @ fb); out["df"].append(dS.T @ gb)
        dS.abs_()
        S["dg1"].append(dS @ fb.abs()); S["df1"].append(dS.T @ gb.abs())
        del dS
        T = hb.abs() @ dyb.abs().T
        T += Sdelta[:, None]                            # sum_j' P_ij' A_ij' = S(delta_i)
        T *= P
        S["dg2"].append(T @ fb.abs()); S["df2"].append(T.T @ gb.abs())
        del T, P
    ref = {k: torch.stack(v) for k, v in out.items()}
    ref["lnZ"] = ref["Z"].log()
    ref["lse"] = ref["m"] + ref["lnZ"]
    ref["S"] = {k: torch.stack(v) for k, v in S.items()}
    ref["S"]["x"] = x.to(device=device, dtype=torch.float64).abs()
    return ref


def slacks(ref, family):
    """family: "f32" | "bf16_valu" | "mfma"  ->  {output: (a half bf16 ulp on top?, slack tensor)}"""
    S = ref["S"]
    bf, mf = family != "f32", family == "mfma"
    k1 = K_P_BF16 if mf else 0.0
    kc = K_CANCEL_MFMA if mf else ACC
    return {"m": (False, ACC * S["m"]),
            "lnZ": (False, LNZ_ABS + ACC * S["sc"]),
            "lse": (False, LNZ_ABS + ACC * S["sc"]),
            "y": (bf, k1 * S["y"] + ACC * (S["y"] + S["x"])),
            "dh": (bf, k1 * S["dh"] + ACC * S["dh"]),
            "delta": (False, (K_DELTA_MFMA if mf else ACC) * S["delta"]),
            "dg": (bf, k1 * S["dg1"] + kc * S["dg2"]),
            "df": (bf, k1 * S["df1"] + kc * S["df2"])}


def check(got, ref, family, where="", ratios=None):
    """every element of every output of `got` (m, Z, y, dh, delta, dg, df: what the kernels stored) inside its bound; the worst
    error / bound of each output is printed first and kept in `ratios` (a dict of maxima, if given)"""
    got = {k: v.to(device=ref["y"].device, dtype=torch.float64) for k, v in got.items()}
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), f"{where} {k}: {int((~torch.isfinite(v)).sum())} of {v.numel()} elements are not finite"
    got["lnZ"] = got["Z"].log()
    got["lse"] = got["m"] + got["lnZ"]
    sl = slacks(ref, family)
    worst = {}
    for k in OUTPUTS:
        half, slack = sl[k]
        tol = slack + 1e-30
        if half:
            tol = tol + 0.5 * ulp_bf16(torch.maximum(got[k].abs(), ref[k].abs())) * (1 + 1e-6)
        worst[k] = float(((got[k] - ref[k]).abs() / tol).max())
        if ratios is not None:
            ratios[(family, k)] = max(ratios.get((family, k), 0.0), worst[k])
    print(f"{where} [{family}] worst err/bound: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    for k in OUTPUTS:
        half, slack = sl[k]
        if half:
            assert_rounded(got[k], ref[k], slack, f"{where} {k}")
        else:
            d = (got[k] - ref[k]).abs()
            bad = d > slack + 1e-30
            assert not bool(bad.any()), (f"{where} {k}: {int(bad.sum())} of {bad.numel()} elements beyond the bound; worst error / bound "
                                         f"{worst[k]:.3g}")
    return worst


def make_inputs(gen, B, N, D, C, seed=0, extent=None, W=None):
    """-> f, g [B, N, D], h, x, dy [B, N, C]: float32 CPU tensors of bf16-representable values (0 outside the extents)"""
    assert gen in GENERATORS, gen
    G = torch.Generator().manual_seed(1000 * seed + 7 * N + D + C + GENERATORS.index(gen))
    rn = lambda *s: torch.randn(*s, generator=G)
    h, x, dy = rn(B, N, C), rn(B, N, C), rn(B, N, C)
    if gen == "peaked":                                # scores of std 12: nearly one-hot rows, delta cancels h . dy at the peak
        sig = (12.0 / D ** 0.5) ** 0.5
        f, g = sig * rn(B, N, D), sig * rn(B, N, D)
    elif gen in ("shift_neg", "shift_pos"):            # a quarter of the rows (and the last three, in the last partial tile) score
        f = 4.0 + 0.5 * rn(B, N, D)                    # -+16 D +- 2 sqrt(D) against EVERY key: -128 +- 6 at D = 8
        g = 0.7 * rn(B, N, D)
        i = torch.arange(N)
        rows = (i % 4 == 1) | (i >= N - 3)
        g[:, rows] = -4.0 if gen == "shift_neg" else 4.0
    else:
        f, g = 0.7 * rn(B, N, D), 0.7 * rn(B, N, D)
    if gen == "f_zero":
        f = torch.zeros_like(f)
    if gen == "h_zero":
        h = torch.zeros_like(h)
    ts = [t.bfloat16().float() for t in (f, g, h, x, dy)]
    if extent is not None:
        for b in range(B):
            inn = extent_mask(extent[b], N, W, "cpu")
            for t in ts:
                t[b, ~inn] = 0
    return ts


def emulate(f, g, h, x, dy, family, extent=None, W=None):
    """The kernels' arithmetic in torch: fp32 sums; "mfma": P and dS rounded to bf16 ahead of the second product and delta taken
    from the unrounded dh sums (of rounded P), as the sweeps do; bf16 families round what they store.  -> what the kernels store."""
    B, N, D = f.shape
    bf, mf = family != "f32", family == "mfma"
    q = (lambda t: t.bfloat16().float()) if mf else (lambda t: t)
    st = (lambda t: t.bfloat16().float()) if bf else (lambda t: t)
    out = {k: [] for k in ("m", "Z", "y", "dh", "delta", "dg", "df")}
    for b in range(B):
        fb, gb, hb, xb, dyb = (t[b].float() for t in (f, g, h, x, dy))
        inn = torch.ones(N, dtype=torch.bool) if extent is None else extent_mask(extent[b], N, W, "cpu")
        s = gb @ fb.T
        s[:, ~inn] = -float("inf")
        m = s.max(1).values
        Z = torch.exp(s - m[:, None]).sum(1)
        P = torch.exp(s - (m + Z.log())[:, None])
        P[~inn] = 0
        Pq = q(P)
        y = xb + Pq.T @ hb
        y[~inn] = xb[~inn]
        dh = Pq @ dyb
        delta = (hb * dh).sum(1)
        dSq = q(P * (hb @ dyb.T - delta[:, None]))
        for k, v in (("m", m), ("Z", Z), ("y", st(y)), ("dh", st(dh)), ("delta", delta), ("dg", st(dSq @ fb)), ("df", st(dSq.T @ gb))):
            out[k].append(v)
    return {k: torch.stack(v) for k, v in out.items()}
