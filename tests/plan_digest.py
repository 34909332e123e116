"""Digest of a lowered plan: pins what `_Plan` emits (op order, shapes, flags, split counts, tile forms, buffer aliasing)
without pinning the allocator.

Every integer and float field of every op of `op_array` and `bwd_array` is hashed verbatim; every pointer field is replaced
by the rank of that exact address in order of first appearance over the whole plan (null stays null).  The recorded digests
live in tests/plan_digests.json; a deliberate lowering change re-records them on the GPU with

    python tests/plan_digest.py --record

and the diff of the op-type strings in the JSON file shows what moved.
"""
import ctypes
import hashlib
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_digests.json")
MEAN = (-455.934, 417.50, 520.31)
BIG = (2, 3, 256, 384)        # F(6x6,3x3) with 96 tiles, pair GEMMs, kept-V weight gradients
SMALL = (1, 3, 64, 96)        # deepest map 8 x 12: no Winograd form, direct and 1x1 kernels


def _cfg(shape, train, env=None, batch_invariant=False, **net):
    return dict(shape=shape, train=train, env=env or {}, batch_invariant=batch_invariant, net=net)


CONFIGS = {}
for _name, _shape in (("64x96", SMALL), ("128x192", (3, 3, 128, 192)), ("256x384", BIG)):
    CONFIGS["base_%s_infer" % _name] = _cfg(_shape, False)
    CONFIGS["base_%s_train" % _name] = _cfg(_shape, True)
CONFIGS["tiny_infer"] = _cfg(SMALL, False, tiny=True)
CONFIGS["tiny_train"] = _cfg(SMALL, True, tiny=True)
CONFIGS["batch_invariant_infer"] = _cfg((2, 3, 64, 96), False, batch_invariant=True)
CONFIGS["mlr3_unfrozen1_train"] = _cfg(SMALL, True, num_mlr=3, num_unfrozen_encoder=1)
CONFIGS["full_size_infer"] = _cfg(SMALL, False, full_size_output=True)
for _key, _val, _modes in (("XL_GEMM_PAIR", "0", (False, True)), ("XL_GEMM_SPLIT_BF16", "0", (False, True)),
                           ("XL_NO_WINOGRAD", "1", (False, True)), ("XL_NO_DEFERRED_GN", "1", (False, True)),
                           ("XL_TRAIN_PAIR_BWD", "0", (True,)), ("XL_WINOGRAD", "4", (False, True))):
    for _train in _modes:
        CONFIGS["%s=%s_%s" % (_key, _val, "train" if _train else "infer")] = _cfg(BIG, _train, env={_key: _val})


def build_net(cfg, device):
    import torch
    from crossloc_amd import networks
    from crossloc_amd.weights import seeded_state_dict
    kw = dict(cfg["net"])
    net = networks.TransPoseNet(torch.tensor(MEAN), kw.pop("tiny", False), False, 1, 1, 3, 1, **kw)
    net.load_state_dict(seeded_state_dict(net))
    net.batch_invariant = cfg["batch_invariant"]
    return net.to(device)


def build_plan(cfg, device):
    """The plan of `cfg` under exactly cfg["env"] (the caller's environment is restored)."""
    from crossloc_amd import networks
    saved = {k: os.environ.get(k) for k in cfg["env"]}
    os.environ.update(cfg["env"])
    try:
        net = build_net(cfg, device)
        B, _, H, W = cfg["shape"]
        return networks._Plan(net, B, H, W, device, train=cfg["train"])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_TYPE_CHARS = "0123456789abcdefghijklmnopqrstuvwxyz"


def plan_digest(plan):
    """{"digest": sha256 hex, "fwd": op types of op_array, "bwd": op types of bwd_array}, one character per op."""
    from crossloc_amd.networks import XlOp
    ranks, h = {}, hashlib.sha256()
    types = {}
    for name in ("op_array", "bwd_array"):
        ops = getattr(plan, name, None) or ()
        types[name] = "".join(_TYPE_CHARS[op.type] for op in ops)
        h.update(struct.pack("<i", len(ops)))
        for op in ops:
            for field, ctype in XlOp._fields_:
                v = getattr(op, field)
                if ctype is ctypes.c_int32:
                    h.update(struct.pack("<i", v))
                elif ctype is ctypes.c_float:
                    h.update(struct.pack("<f", v))
                else:
                    h.update(struct.pack("<q", ranks.setdefault(v, len(ranks) + 1) if v else 0))
    return {"digest": h.hexdigest(), "fwd": types["op_array"], "bwd": types["bwd_array"]}


def compute_all(device):
    return {name: plan_digest(build_plan(cfg, device)) for name, cfg in CONFIGS.items()}


def main(argv):
    import torch
    if "--record" not in argv:
        sys.exit("usage: python tests/plan_digest.py --record   (on the GPU; rewrites tests/plan_digests.json)")
    out = argv[argv.index("--out") + 1] if "--out" in argv else RECORD
    with open(out, "w") as f:
        json.dump(compute_all(torch.device("cuda:0")), f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d plan digests in %s" % (len(CONFIGS), out))


if __name__ == "__main__":
    main(sys.argv[1:])
