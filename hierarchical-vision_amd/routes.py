"""Which libhvk kernel family takes a GEMM-shaped op: one pure function per decision.

Each takes plain integers, reads options.OPTIONS and libhvk's hvk_*_supported queries, and returns
a short string, or None where no hand-written kernel applies (the caller then takes its unfused
form or leaves libhvk through ops.library_fallback).  ops.py only switches on the answers, and
tests/test_routes_cpu.py pins the whole table (tests/golden/routes_golden.json): a new kernel form
changes one line here and one diff of that table.  Answers are cached per (shape, routing
options), so a product call crosses ctypes at most once per query and shape.
"""
from . import _lib
from .options import OPTIONS

DW_TOK = 32  # tokens per stage of libhvk's weight-gradient kernel (csrc/gemm_tn.hip TOK)
_CACHE = {}
clear = _CACHE.clear  # forget every answer (the routing-table recorder replaces libhvk's queries)


def _q(name, *shape):
    """libhvk's `name`(*shape) as a bool: a pure function of the shape within one process."""
    r = _CACHE.get((name, shape))
    if r is None:
        r = _CACHE[(name, shape)] = bool(getattr(_lib.load(), name)(*shape))
    return r


def _route(fn):
    """Cache fn(*shape) per shape and value of every option a route reads."""
    def route(*shape):
        o = OPTIONS
        key = (fn, shape, o.skinny_b, o.s1_gelu_tile, o.mlp_fused, o.gelu_recompute, o.ln_epilogue,
               o.ln_epilogue_tile, o.merge_gemm)
        try:
            return _CACHE[key]
        except KeyError:
            r = _CACHE[key] = fn(*shape)
            return r
    route.__doc__ = fn.__doc__
    return route


def tile_any(M, K, N):
    """libhvk's tiled GEMM takes the shape at all (hvk_gemm_supported: K % 64, 128 | N or 192 | N,
    any M): the native route for shapes outside the measured speed rules of tile_ok and the
    skinny kernel's table (small microbatches), instead of the library GEMM."""
    return M > 0 and _q("hvk_gemm_supported", 1, K, N)


def skinny(M, K, N):
    """libhvk's skinny MFMA GEMM is built for (K, N) (include/hvk.h)."""
    return M > 0 and _q("hvk_linear_supported", 1, K, N)


def tile_ok(M, K, N):
    """libhvk's tiled MFMA GEMM (hvk_gemm_fwd) where it measured faster than the library GEMM
    (tools/bench_gemm.py): the stage-2 shapes (K <= 1536, fc2 forward and fc1 input gradient
    included), the stage-1 shapes with 192 | N (K >= 192), and every stage-3 shape (and the
    stage-2 PatchMerging) with 192 | N, on 128 x 192 tiles."""
    if K % 64 or M <= 0:
        return False
    if N % 128:  # the 128 x 192 tile: stage-1 qkv / proj / fc2 forward, qkv / fc1 input grads
        return N % 192 == 0 and K >= 192 and M >= 32768
    if M >= 8192 and N % 192 == 0:  # stage 3 and its PatchMerging (128 x 192 tiles)
        return True
    return (M >= 32768 and K <= 1536) or (K == 768 and N == 768)


def _skinny_first_k():
    """SwinV2-B's stage 0-1 widths (K = 128 / 256): the skinny kernel before the tiled one."""
    return (128, 256) if OPTIONS.skinny_b else ()


def _gelu_skinny_k():
    """fc1 + GELU widths on the skinny kernel: stage 0 outside the fused MLP; stage 1 unless
    options.s1_gelu_tile routes it to the tiled EPI 1 kernel; the skinny-first widths."""
    return ((96,) if OPTIONS.s1_gelu_tile else (96, 192)) + _skinny_first_k()


def _tile_or_skinny(M, K, N, sk):
    """x W^T with a skinny form built (`sk`) or not: the tile where it measured faster (unless the
    width is skinny-first) or is the only kernel, else the skinny kernel, else None."""
    if (tile_ok(M, K, N) and not (K in _skinny_first_k() and skinny(M, K, N))) or (not sk and tile_any(M, K, N)):
        return "tile"
    return "skinny" if sk else None


@_route
def nt(M, K, N):
    """y = x W^T, x [M, K], W [N, K] (an input gradient g W is nt(M, N, K)): "tile" (hvk_gemm_fwd),
    "skinny" (hvk_linear_fwd) or None (the library GEMM)."""
    return _tile_or_skinny(M, K, N, skinny(M, K, N))


@_route
def qkv(M, K, N):
    """The qkv Linear with the q / k normalisation in its epilogue: "tile" (hvk_gemm_qkv_fwd),
    "skinny" (hvk_linear_qkv_fwd) or "normalize" (nt's GEMM + hvk_qk_normalize)."""
    sk = skinny(M, K, N) and _q("hvk_linear_qkv_supported", M, K, N)
    return (_tile_or_skinny(M, K, N, sk) if N % 96 == 0 else "skinny" if sk else None) or "normalize"


@_route
def gelu_fwd(M, K, N):
    """fc1 + bias + GELU as one kernel: "skinny" (hvk_linear_gelu_fwd), "tile" (hvk_gemm_gelu_fwd)
    or None (GEMM + activation kernel)."""
    if K in _gelu_skinny_k() and _q("hvk_linear_gelu_supported", M, K, N):
        return "skinny"
    return "tile" if tile_any(M, K, N) else None


@_route
def gelu_bwd(M, N2, N1):
    """fc2's input gradient through GELU' as one kernel (g [M, N2], h [M, N1]): "tile"
    (hvk_gemm_gelu_bwd), "skinny" (hvk_linear_gelu_bwd) or None."""
    sk = _q("hvk_linear_gelu_bwd_supported", M, N2, N1)
    if not sk:
        return "tile" if tile_any(M, N2, N1) else None
    return "tile" if tile_ok(M, N2, N1) and N2 not in _skinny_first_k() else "skinny"


@_route
def mlp(M, K, N1, N2):
    """MlpFn's plan for fc2(GELU(fc1(x))), x [M, K]: "recompute" (options.gelu_recompute, stage 0:
    only h is kept and fc2 and its weight gradient recompute GELU(h); bit-identical, off by
    default: on MI355X it costs fc2 +80 us and the weight gradient +217 us against the 233 us the
    y write saves), "fused" (hvk_mlp_fwd, stage 0), "chain" (gelu_fwd + nt) or None (no fused
    fc1 + GELU or GELU' kernel: linear_gelu + linear)."""
    if gelu_fwd(M, K, N1) is None or gelu_bwd(M, N2, N1) is None:
        return None
    if (OPTIONS.gelu_recompute and skinny(M, K, N1) and _q("hvk_linear_gelu_in_supported", M, N1, N2)
            and _q("hvk_weight_grad_gelu_x_supported", M, N2, N1)):
        return "recompute"
    return "fused" if OPTIONS.mlp_fused and _q("hvk_mlp_fwd_supported", M, K, N1, N2) else "chain"


@_route
def mlp_bwd_fused(M, K, N1, N2):
    """Both input gradients of the MLP as one kernel (hvk_mlp_bwd, stage 0), for a plan that kept
    GELU(h) and a wanted input gradient; else gelu_bwd + nt."""
    return OPTIONS.mlp_fused and _q("hvk_mlp_bwd_supported", M, N2, N1, K)


@_route
def linear_ln(M, K, N):
    """"ln": the Linear + post-norm epilogue (hvk_linear_ln_fwd) is built for the shape and enabled
    (options.ln_epilogue; the C = 192 tile form also options.ln_epilogue_tile); else None."""
    on = OPTIONS.ln_epilogue and (N == 96 or OPTIONS.ln_epilogue_tile)
    return "ln" if on and _q("hvk_linear_ln_supported", M, K, N) else None


@_route
def mlp_ln(M, K, N1, N2):
    """MlpLNFn's plan: "fused" (hvk_mlp_ln_fwd and the fused backward, stage 0), "chain" (gelu_fwd,
    then fc2 on the tile's LN epilogue) or None (MlpFn + a separate norm)."""
    if not OPTIONS.ln_epilogue:
        return None
    if _q("hvk_mlp_ln_supported", M, K, N1, N2) and mlp_bwd_fused(M, K, N1, N2):
        return "fused"
    return "chain" if N2 != 96 and linear_ln(M, N1, N2) and mlp(M, K, N1, N2) in ("fused", "chain") else None


@_route
def merge(B, H, W, C, N):
    """PatchMerging's gather folded into its reduction GEMM both ways (hvk_merge_*; options
    merge_gemm): "ln" with the norm in the epilogue too (N = 192; ln_epilogue, ln_epilogue_tile),
    "gemm" without, or None."""
    if not (OPTIONS.merge_gemm and _q("hvk_merge_gemm_supported", B, H, W, C, N)
            and _q("hvk_merge_weight_grad_supported", B, H, W, C, N)):
        return None
    ln = OPTIONS.ln_epilogue and OPTIONS.ln_epilogue_tile and _q("hvk_merge_linear_ln_supported", B, H, W, C, N)
    return "ln" if ln else "gemm"


@_route
def dw(M, N, K, gelu_x=False):
    """libhvk's weight-gradient kernel takes the shape: directly when 32 | M, else as a main launch
    over the first M - M % 32 tokens plus one over the zero-padded 32-token tail."""
    name = "hvk_weight_grad_gelu_x_supported" if gelu_x else "hvk_weight_grad_supported"
    return M > 0 and _q(name, M - M % DW_TOK if M >= DW_TOK else DW_TOK, N, K)
