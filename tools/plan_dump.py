"""Dump the launch lists of a set of plans as JSON, or compare two such dumps.

    python tools/plan_dump.py [--device cpu|cuda] [--pkg-root DIR] [--descriptors] > plans.json
    python tools/plan_dump.py --diff parent.json branch.json [--allow-count KEY ...]

For every plan below: the ordered forward and backward lists of (kind, key, bytes) and `launch_meta`.  Only
`plan._fwd_seq`, `plan._bwd_seq`, `plan.rec_meta` and `plan.launch_meta` are read, so the same file runs against any
revision of `msau_amd` (--pkg-root: the directory that holds the `msau_amd` package to import, with its built library) --
the way to diff the plan of a fusion change against its parent.  Plans build on the CPU (no kernel runs); some host-side
instance choices may depend on a device, hence --device.

--descriptors: also the full content of every launch record's argument struct (`fwd_desc`, `bwd_desc`) and the plan's
`_pack_entries`, `_unpack_entries` and `_unpack_stage`.  The struct type follows from the record's kind through the ctypes
mirrors of msau_amd/_lib.py (an unknown kind is an error).  Integers verbatim, floats as their bit pattern, pointers as
[allocation, byte offset]: the allocations are the storages of the torch tensors alive once the plan is built, named by their
ordinal in order of first use (forward list, backward list, struct field order), so two builds at different addresses give the
same dump.  Null is null; a pointer into no allocation is an error (a placeholder that was never patched).

--diff: the lists must be identical (a record without a key on either side compares on its kind alone); `launch_meta` key
by key, counts exactly, bytes and flops to a relative 1e-12 (the order of a float sum).  --allow-count KEY: the count of
KEY may differ (its bytes and flops still may not).  Descriptor dumps compare exactly, field by field: no allowed differences.
Exit status 1 when anything differs.
"""
import argparse
import bisect
import ctypes
import gc
import json
import os
import struct
import sys
import time
import warnings

BASE = dict(channels=64, n_class=5, scale_space_num=4, res_depth=2, featRoot=8, filter_size=3, pool_size=2, num_blocks=3)
GEOM = {"cfg1": (dict(channels=32, num_blocks=1), 2, 128, 128), "cfg2": (dict(), 2, 336, 256),
        "cfg4": (dict(channels=768, num_blocks=2), 1, 336, 256), "cfg5": (dict(), 1, 512, 384),
        "small": (dict(channels=13), 1, 33, 26)}
DESC_KEYS = ("fwd_desc", "bwd_desc", "pack", "unpack", "unpack_stage")


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


def build_plan(case, device):
    import torch
    from msau_amd import _lib as L
    from msau_amd.model import param_shapes
    from msau_amd.plan import Plan
    name, over, B, H, W, dt, kw = case
    cfg = dict(BASE, **over)
    shapes = param_shapes(cfg)
    poff, off = {}, 0
    for k, s in shapes.items():
        n = 1
        for d in s:
            n *= int(d)
        poff[k] = off
        off += -(-n // 4) * 4
    return Plan(cfg, B, H, W, L.F32 if dt == "f32" else L.BF16, torch.device(device), poff, dict(shapes), **kw)


def launch_lists(plan):
    ent = {}
    for tag, seq in (("fwd", plan._fwd_seq), ("bwd", plan._bwd_seq)):
        rows = []
        if seq is not None:
            for i in range(seq[1]):
                key, nbytes = plan.rec_meta.get(seq[0][i].args) or (None, None)
                rows.append([int(seq[0][i].kind), key, nbytes])
        ent[tag] = rows
    ent["launch_meta"] = {k: list(v) for k, v in plan.launch_meta.items()}
    return ent


def struct_of_kind(L):
    return {L.OP_CONV2D: L.ConvDesc, L.OP_WGRAD: L.WgradDesc, L.OP_LRN_FWD: L.LrnArgs, L.OP_LRN_BWD: L.LrnArgs,
            L.OP_POOL_FWD: L.PoolArgs, L.OP_POOL_BWD: L.PoolArgs, L.OP_ATTN_FWD: L.AttnArgs, L.OP_ATTN_BWD: L.AttnArgs,
            L.OP_CHANNEL_SUM: L.CsumArgs, L.OP_WGRAD_REDUCE: L.ReduceArgs, L.OP_CONV_PAIR: L.ConvPairDesc,
            L.OP_BOX_FWD: L.BoxArgs, L.OP_BOX_BWD: L.BoxArgs, L.OP_ATTN_PROJ_BWD: L.AttnProjBwdArgs,
            L.OP_DGRAD2_1X1: L.Dgrad2Args}


def live_allocations():
    """sorted [(first byte, one past the last byte)] of the storages of every torch tensor alive now"""
    import torch
    spans = set()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # (isinstance touches every object alive, deprecated aliases included)
        for o in gc.get_objects():
            if isinstance(o, torch.Tensor):
                st = o.untyped_storage()
                if st.nbytes():
                    spans.add((st.data_ptr(), st.data_ptr() + st.nbytes()))
    return sorted(spans)


def fields_of(s, where, resolve=None):
    """{field: value} of a ctypes struct; a pointer field goes through `resolve` (a struct of offsets only has none)"""
    out = {}
    for name, ctype in s._fields_:
        v = getattr(s, name)
        if ctype is ctypes.c_void_p:
            v = resolve(v, f"{where}.{name}")
        elif ctype is ctypes.c_float:
            v = struct.unpack("<I", struct.pack("<f", v))[0]
        out[name] = v
    return out


def descriptors(plan):
    """every launch record's argument struct, and the pack / unpack tables, free of addresses"""
    from msau_amd import _lib as L
    types = struct_of_kind(L)
    spans = live_allocations()
    starts = [a for a, _ in spans]
    names = {}

    def resolve(p, where):
        if not p:
            return None
        i = bisect.bisect_right(starts, p) - 1
        if i < 0 or p >= spans[i][1]:
            raise ValueError(f"{where} = {p:#x} lies in no live allocation (a placeholder that was never patched?)")
        return [names.setdefault(spans[i][0], len(names)), p - spans[i][0]]

    ent = {}
    for tag, seq in (("fwd", plan._fwd_seq), ("bwd", plan._bwd_seq)):
        rows = []
        for i in range(seq[1] if seq is not None else 0):
            kind = int(seq[0][i].kind)
            if kind & 0xff not in types:
                raise ValueError(f"{tag}[{i}]: unknown launch kind {kind & 0xff} ({kind:#x})")
            T = types[kind & 0xff]
            rows.append({"kind": kind, "type": T.__name__,
                         "fields": fields_of(T.from_address(seq[0][i].args), f"{tag}[{i}] {T.__name__}", resolve)})
        ent[tag + "_desc"] = rows
    ent["pack"] = [fields_of(e, f"pack[{i}]") for i, e in enumerate(plan._pack_entries)]
    ent["unpack"] = [fields_of(e, f"unpack[{i}]") for i, e in enumerate(plan._unpack_entries)]
    ent["unpack_stage"] = [int(s) for s in plan._unpack_stage]
    return ent


def dump(device, with_descriptors=False):
    res = {}
    for case in cases():
        t0 = time.perf_counter()
        plan = build_plan(case, device)
        ent = {"build_s": round(time.perf_counter() - t0, 4)}
        ent.update(launch_lists(plan))
        if with_descriptors:
            try:
                ent.update(descriptors(plan))
            except ValueError as e:
                raise SystemExit(f"{case[0]}: {e}")
        res[case[0]] = ent
    return res


def close(a, b):
    return a == b or abs(a - b) <= 1e-12 * max(abs(a), abs(b))


def diff_descriptors(name, a, b, bad):
    """exact, field by field; `a` and `b` are one plan's entries of two --descriptors dumps"""
    for tag in ("fwd_desc", "bwd_desc", "pack", "unpack"):
        if len(a[tag]) != len(b[tag]):
            bad.append(f"{name} {tag}: {len(a[tag])} records against {len(b[tag])}")
            continue
        for i, (ra, rb) in enumerate(zip(a[tag], b[tag])):
            if tag.endswith("_desc"):
                for k in ("kind", "type"):
                    if ra[k] != rb[k]:
                        bad.append(f"{name} {tag}[{i}] {k}: {ra[k]} against {rb[k]}")
                ra, rb = ra["fields"], rb["fields"]
            for k in list(ra) + [k for k in rb if k not in ra]:
                if k not in ra or k not in rb or ra[k] != rb[k]:
                    bad.append(f"{name} {tag}[{i}] {k}: {ra.get(k, 'absent')} against {rb.get(k, 'absent')}")
    if a["unpack_stage"] != b["unpack_stage"]:
        bad.append(f"{name} unpack_stage: {a['unpack_stage']} against {b['unpack_stage']}")


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
        has = [all(k in e for k in DESC_KEYS) for e in (a, b)]
        if has[0] != has[1]:
            bad.append(f"{name}: descriptors in only one of the dumps")
        elif has[0]:
            diff_descriptors(name, a, b, bad)
    for ln in bad:
        print(ln)
    print(f"{len(set(A) & set(B))} plans compared, {len(bad)} differences")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--pkg-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--descriptors", action="store_true")
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    ap.add_argument("--allow-count", nargs="*", default=[])
    args = ap.parse_args()
    if args.diff:
        sys.exit(diff(args.diff[0], args.diff[1], set(args.allow_count)))
    sys.path.insert(0, os.path.abspath(args.pkg_root))
    json.dump(dump(args.device, args.descriptors), sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
