"""Dump the launch lists of a set of plans as JSON, or compare two such dumps.

    python tools/plan_dump.py [--device cpu|cuda] [--pkg-root DIR] > plans.json
    python tools/plan_dump.py --diff parent.json branch.json [--allow-count KEY ...]

For every plan below: the ordered forward and backward lists of (kind, key, bytes) and `launch_meta`.  Only
`plan._fwd_seq`, `plan._bwd_seq`, `plan.rec_meta` and `plan.launch_meta` are read, so the same file runs against any
revision of `msau_amd` (--pkg-root: the directory that holds the `msau_amd` package to import, with its built library) --
the way to diff the plan of a fusion change against its parent.  Plans build on the CPU (no kernel runs); some host-side
instance choices may depend on a device, hence --device.

--diff: the lists must be identical (a record without a key on either side compares on its kind alone); `launch_meta` key
by key, counts exactly, bytes and flops to a relative 1e-12 (the order of a float sum).  --allow-count KEY: the count of
KEY may differ (its bytes and flops still may not).  Exit status 1 when anything differs.
"""
import argparse
import json
import os
import sys
import time

BASE = dict(channels=64, n_class=5, scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, num_blocks=3)
GEOM = {"cfg1": (dict(channels=32, num_blocks=1), 2, 128, 128), "cfg2": (dict(), 2, 336, 256),
        "cfg4": (dict(channels=768, num_blocks=2), 1, 336, 256), "cfg5": (dict(), 1, 512, 384),
        "small": (dict(channels=13), 1, 33, 26)}


def cases():
    """(name, cfg overrides, B, H, W, dtype name, Plan keyword arguments)"""
    out = [(f"{g}.{dt}.train", c, B, H, W, dt, {}) for g, (c, B, H, W) in GEOM.items() for dt in ("f32", "bf16")]
    c, B, H, W = GEOM["cfg2"]
    out += [("cfg2.bf16.infer.reuse", dict(reuse_activations=True), B, H, W, "bf16", dict(training=False)),
            ("cfg2.bf16.infer.noreuse", dict(reuse_activations=False), B, H, W, "bf16", dict(training=False)),
            ("cfg2.bf16.ragged", {}, B, H, W, "bf16", dict(ragged=True)),
            ("cfg2.bf16.elu", dict(activation="elu"), B, H, W, "bf16", {})]
    out += [(f"cfg2.bf16.{k}=False", {k: False}, B, H, W, "bf16", {}) for k in ("fuse_pair", "fuse_couple", "overlap_wgrad")]
    return out


def dump(device):
    import torch
    from msau_amd import _lib as L
    from msau_amd.model import param_shapes
    from msau_amd.plan import Plan
    res = {}
    for name, over, B, H, W, dt, kw in cases():
        cfg = dict(BASE, **over)
        shapes = param_shapes(cfg)
        poff, off = {}, 0
        for k, s in shapes.items():
            n = 1
            for d in s:
                n *= int(d)
            poff[k] = off
            off += -(-n // 4) * 4
        t0 = time.perf_counter()
        plan = Plan(cfg, B, H, W, L.F32 if dt == "f32" else L.BF16, torch.device(device), poff, dict(shapes), **kw)
        ent = {"build_s": round(time.perf_counter() - t0, 4)}
        for tag, seq in (("fwd", plan._fwd_seq), ("bwd", plan._bwd_seq)):
            rows = []
            if seq is not None:
                for i in range(seq[1]):
                    key, nbytes = plan.rec_meta.get(seq[0][i].args) or (None, None)
                    rows.append([int(seq[0][i].kind), key, nbytes])
            ent[tag] = rows
        ent["launch_meta"] = {k: list(v) for k, v in plan.launch_meta.items()}
        res[name] = ent
    return res


def close(a, b):
    return a == b or abs(a - b) <= 1e-12 * max(abs(a), abs(b))


def diff(pa, pb, allow_count):
    A, B = json.load(open(pa)), json.load(open(pb))
    bad = []
    if sorted(A) != sorted(B):
        bad.append(f"plans differ: {sorted(set(A) ^ set(B))}")
    for name in sorted(set(A) & set(B)):
        a, b = A[name], B[name]
        for tag in ("fwd", "bwd"):
            if len(a[tag]) != len(b[tag]):
                bad.append(f"{name} {tag}: {len(a[tag])} records against {len(b[tag])}")
                continue
            for i, (ra, rb) in enumerate(zip(a[tag], b[tag])):
                same = ra[0] == rb[0] if ra[1] is None or rb[1] is None else ra == rb
                if not same:
                    bad.append(f"{name} {tag}[{i}]: {ra} against {rb}")
        ma, mb = a["launch_meta"], b["launch_meta"]
        for k in sorted(set(ma) | set(mb)):
            if k not in ma or k not in mb:
                bad.append(f"{name} launch_meta[{k}]: {ma.get(k)} against {mb.get(k)}")
                continue
            (na, ba, fa), (nb, bb, fb) = ma[k], mb[k]
            if (na != nb and k not in allow_count) or not close(ba, bb) or not close(fa, fb):
                bad.append(f"{name} launch_meta[{k}]: {ma[k]} against {mb[k]}")
    for ln in bad:
        print(ln)
    print(f"{len(set(A) & set(B))} plans compared, {len(bad)} differences")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--pkg-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    ap.add_argument("--allow-count", nargs="*", default=[])
    args = ap.parse_args()
    if args.diff:
        sys.exit(diff(args.diff[0], args.diff[1], set(args.allow_count)))
    sys.path.insert(0, os.path.abspath(args.pkg_root))
    json.dump(dump(args.device), sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
