"""The routing table of hvamd.ops: which hvk_* entry points each GEMM-family op launches, in
order, forward and backward, over every SwinV2-T / -S / -B width, the token counts around each
routing threshold and every combination of the routing options.

    python tests/golden/make_routes_golden.py CHECKOUT [OUT.json]

records the table of the checkout at CHECKOUT (a built tree: libhvk.so is loaded for its
hvk_*_supported queries) into OUT.json (default: routes_golden.json beside this script).  The
committed table is recorded from the PARENT of the commit that changes the routing, never from
the code under test: tests/test_routes_cpu.py replays `record` on the tree it runs in and
requires equality for every key.

No GPU is needed: the ops run on device="meta" tensors with ops.call / ptr / stream /
library_fallback replaced by recorders, so only the launch decisions execute.  The three fused
stage-0 MLP queries (hvk_mlp_fwd / _ln / _bwd_supported) also ask the device for ~149 KB of LDS
and answer 0 without one; they are replaced by their shape predicate, i.e. the table is the one
of a device that grants it (MI355X).  A refusing device routes like options.mlp_fused = False,
which the grid holds as well.
"""
import contextlib
import itertools
import json
import os
import sys

WIDTHS = (96, 128, 192, 256, 384, 512, 768, 1024)
TOKENS = (49, 1568, 8192, 9408, 32768, 200704)
BASE = ("s1_gelu_tile", "skinny_b", "mlp_fused", "gelu_recompute")
LN = BASE + ("ln_epilogue", "ln_epilogue_tile")
MERGE = ("merge_gemm", "ln_epilogue", "ln_epilogue_tile")
MERGE_HW = (56, 28, 14)
MERGE_B = (1, 48)
FIXED = dict(wgrad_stream=False, strict_native=False, prepare_weights=True)
GATED_OFF = ("-",)  # the op's *_supported gate said no: nothing launched


def _t(torch, shape, dtype=None, grad=True):
    return torch.empty(shape, device="meta", dtype=dtype or torch.float32, requires_grad=grad)


def _backward(torch, outs):
    outs = [o for o in (outs if isinstance(outs, tuple) else (outs,)) if o.requires_grad]
    torch.autograd.backward(outs, [torch.empty_like(o) for o in outs])


def _linear(kn):
    def run(torch, ops, M, C):
        K, N = kn(C)
        _backward(torch, ops.linear(_t(torch, (M, K), torch.bfloat16), _t(torch, (N, K)), _t(torch, (N,))))
    return run


def _linear_qkv(torch, ops, M, C):
    y, _ = ops.linear_qkv(_t(torch, (M, C), torch.bfloat16), _t(torch, (3 * C, C)), _t(torch, (3 * C,), grad=False),
                          _t(torch, (C // 32,)))
    _backward(torch, y)


def _linear_gelu(torch, ops, M, C):
    _backward(torch, ops.linear_gelu(_t(torch, (M, C), torch.bfloat16), _t(torch, (4 * C, C)), _t(torch, (4 * C,))))


def _mlp(want_x):
    def run(torch, ops, M, C):
        _backward(torch, ops.mlp(_t(torch, (M, C), torch.bfloat16, want_x), _t(torch, (4 * C, C)), _t(torch, (4 * C,)),
                                 _t(torch, (C, 4 * C)), _t(torch, (C,))))
    return run


def _linear_ln(kn):
    def run(torch, ops, M, C):
        K, N = kn(C)
        if not ops.linear_ln_supported(M, K, N):
            return GATED_OFF
        _backward(torch, ops.linear_ln(_t(torch, (M, K), torch.bfloat16), _t(torch, (N, K)), _t(torch, (M, N)),
                                       _t(torch, (N,)), _t(torch, (N,)), abias=_t(torch, (N,))))
    return run


def _mlp_ln(want_x):
    def run(torch, ops, M, C):
        if not ops.mlp_ln_supported(M, C, 4 * C, C):
            return GATED_OFF
        _backward(torch, ops.mlp_ln(_t(torch, (M, C), torch.bfloat16, want_x), _t(torch, (4 * C, C)),
                                    _t(torch, (4 * C,)), _t(torch, (C, 4 * C)), _t(torch, (M, C)), _t(torch, (C,)),
                                    _t(torch, (C,)), abias=_t(torch, (C,))))
    return run


# op -> (the options its grid varies, runner); the linear shapes are (K, N) of a block of width C
OPS = {
    "linear:proj": (BASE, _linear(lambda C: (C, C))),
    "linear:qkv": (BASE, _linear(lambda C: (C, 3 * C))),
    "linear:fc1": (BASE, _linear(lambda C: (C, 4 * C))),
    "linear:fc2": (BASE, _linear(lambda C: (4 * C, C))),
    "linear:merge": (BASE, _linear(lambda C: (4 * C, 2 * C))),
    "linear_qkv": (BASE, _linear_qkv),
    "linear_gelu": (BASE, _linear_gelu),
    "mlp": (BASE, _mlp(True)),
    "mlp:no_gx": (BASE, _mlp(False)),
    "linear_ln:proj": (LN, _linear_ln(lambda C: (C, C))),
    "linear_ln:merge": (LN, _linear_ln(lambda C: (4 * C, 2 * C))),
    "mlp_ln": (LN, _mlp_ln(True)),
    "mlp_ln:no_gx": (LN, _mlp_ln(False)),
}
LINEAR_KN = {"proj": lambda C: (C, C), "qkv": lambda C: (C, 3 * C), "fc1": lambda C: (C, 4 * C),
             "fc2": lambda C: (4 * C, C), "merge": lambda C: (4 * C, 2 * C)}


def combos(names):
    return [dict(zip(names, bits)) for bits in itertools.product((False, True), repeat=len(names))]


def key(op, C, M, combo):
    return f"{op} C={C} M={M} " + "".join("01"[v] for v in combo.values())


@contextlib.contextmanager
def recording(ops):
    """Inside: ops.call / library_fallback append to the yielded list instead of launching, ptr and
    stream are stubs, and the three LDS-granting queries answer by shape (module docstring)."""
    lib = ops._lib.load()
    log = []
    patched = {"call": lambda name, *a: log.append(name), "ptr": lambda t: None, "stream": lambda: None,
               "library_fallback": lambda site, detail="": log.append("fb:" + site)}
    saved = {n: getattr(ops, n) for n in patched}
    grants = ("hvk_mlp_fwd_supported", "hvk_mlp_ln_supported", "hvk_mlp_bwd_supported")
    saved_lib = {n: getattr(lib, n) for n in grants}
    clear = getattr(getattr(ops, "routes", None), "clear", lambda: None)  # cached answers of the real queries
    try:
        for n, f in patched.items():
            setattr(ops, n, f)
        for n in grants:  # all three are called with (M, 96, 384, 96) at the stage-0 width
            setattr(lib, n, lambda M, K, N1, N2: int(M > 0 and K == 96 and N1 == 384 and N2 == 96))
        clear()
        yield log
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
        for n, f in saved_lib.items():
            setattr(lib, n, f)
        clear()


def record(ops, options):
    """({key: tuple of entry-point names ("fb:<site>" for a library fallback, "raise:<Error>" where
    the op raised, GATED_OFF where its gate declined)} for the whole grid, {merge key:
    (merge_linear_supported, merge_linear_ln_supported)}) of the `ops` / `options` modules given."""
    import torch

    table, merge = {}, {}
    with recording(ops) as log:
        for op, (names, run) in OPS.items():
            for combo in combos(names):
                with options.override(**combo, **FIXED):
                    for C in WIDTHS:
                        for M in TOKENS:
                            del log[:]
                            try:
                                seq = run(torch, ops, M, C) or tuple(log)
                            except Exception as e:  # noqa: BLE001 -- the table records that it raised
                                seq = ("raise:" + type(e).__name__,)
                            table[key(op, C, M, combo)] = seq
        for combo in combos(MERGE):
            with options.override(**combo, **FIXED):
                for C in WIDTHS:
                    for hw in MERGE_HW:
                        for B in MERGE_B:
                            merge[key(f"merge B={B} H={hw}", C, B * hw * hw // 4, combo)] = (
                                bool(ops.merge_linear_supported(B, hw, hw, C, 2 * C)),
                                bool(ops.merge_linear_ln_supported(B, hw, hw, C, 2 * C)))
    return table, merge


def pack(table, merge):
    """The compact JSON form: entry points and launch sequences as indices, one row of
    len(WIDTHS) * len(TOKENS) sequence indices per (op, option combination), equal rows shared."""
    names, seqs, rows, out = {}, {}, {}, {}
    for op, (opts, _) in OPS.items():
        out[op] = []
        for combo in combos(opts):
            row = []
            for C in WIDTHS:
                for M in TOKENS:
                    seq = tuple(names.setdefault(n, len(names)) for n in table[key(op, C, M, combo)])
                    row.append(seqs.setdefault(seq, len(seqs)))
            out[op].append(rows.setdefault(tuple(row), len(rows)))
    mrows = []
    for combo in combos(MERGE):
        mrows.append("".join(str(a + 2 * b) for a, b in (merge[key(f"merge B={B} H={hw}", C, B * hw * hw // 4, combo)]
                                                        for C in WIDTHS for hw in MERGE_HW for B in MERGE_B)))
    return {"entry_points": list(names), "sequences": [list(s) for s in seqs], "rows": [list(r) for r in rows],
            "ops": out, "merge": mrows}


def unpack(packed):
    names, seqs, rows = packed["entry_points"], packed["sequences"], packed["rows"]
    table, merge = {}, {}
    for op, (opts, _) in OPS.items():
        for combo, r in zip(combos(opts), packed["ops"][op]):
            cells = iter(rows[r])
            for C in WIDTHS:
                for M in TOKENS:
                    table[key(op, C, M, combo)] = tuple(names[i] for i in seqs[next(cells)])
    for combo, row in zip(combos(MERGE), packed["merge"]):
        cells = iter(row)
        for C in WIDTHS:
            for hw in MERGE_HW:
                for B in MERGE_B:
                    v = int(next(cells))
                    merge[key(f"merge B={B} H={hw}", C, B * hw * hw // 4, combo)] = (bool(v & 1), bool(v & 2))
    return table, merge


def main(argv):
    checkout = os.path.abspath(argv[1])
    out = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "routes_golden.json")
    sys.path.insert(0, checkout)
    import hvamd.ops as ops
    from hvamd import options
    assert os.path.dirname(os.path.abspath(ops.__file__)).startswith(checkout), ops.__file__
    table, merge = record(ops, options)
    with open(out, "w") as f:
        json.dump(pack(table, merge), f, separators=(",", ":"))
        f.write("\n")
    raised = sorted(k for k, v in table.items() if v[0].startswith("raise"))
    print(f"{len(table)} routes + {len(merge)} merge gates -> {out}; raised: {raised or 'none'}; "
          f"fallbacks: {sum(any(n.startswith('fb:') for n in v) for v in table.values())}")


if __name__ == "__main__":
    main(sys.argv)
