"""CPU-only checks of the linear probe: the fold assignment and the restatement's scaler against
what scikit-learn recorded (tests/golden/linear_probe_golden.npz), the hvk_lp_* exports and their
argument validation (which runs before any HIP call), and the Python surface's refusals."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import linear_probe_ref as ref

HVK_OK, HVK_EINVAL = 0, 1
FOLD_CASES = ("equal", "unequal", "small_class", "singleton", "strings_order")
CASES = ("small", "wide")


# --------------------------------------------------------------------------- folds and scaler
@pytest.mark.parametrize("name", FOLD_CASES)
def test_stratified_folds_equal_sklearn(golden, name):
    from hvamd import linear_probe
    g = golden("linear_probe_golden")
    y, want = g[f"folds.{name}.y"], g[f"folds.{name}.test"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        got = linear_probe.stratified_folds(y, 5)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(ref.stratified_folds(y, 5), want)


@pytest.mark.parametrize("case", CASES)
def test_fixture_folds_and_scaler(golden, case):
    from hvamd import linear_probe
    g = golden("linear_probe_golden")
    L, D = int(g[f"{case}.n_classes"]), int(g[f"{case}.D"])
    Xtr, ytr, Xev, yev = ref.blobs(L, D, g[f"{case}.per_class"], float(g[f"{case}.sep"]), int(g[f"{case}.seed"]),
                                   int(g[f"{case}.n_eval"]))
    assert np.array_equal(ytr, g[f"{case}.ytrain"])
    assert np.array_equal(linear_probe.stratified_folds(ytr, 5), g[f"{case}.folds"])
    mean, scale = ref.scaler(Xtr)
    assert np.allclose(mean, g[f"{case}.scaler_mean"], rtol=1e-12, atol=1e-12)
    assert np.allclose(scale, g[f"{case}.scaler_scale"], rtol=1e-12)
    # what the generator established about the inputs
    acc = g[f"{case}.ref_acc"]
    assert acc.shape == (5,) and acc.min() >= 0.6 and acc.max() <= 0.95
    assert float(g[f"{case}.restatement_acc"]) >= acc.min() + 0.03
    assert g[f"{case}.ref_preds"].shape == (5, len(yev))


def test_stratified_folds_raise_and_warn_as_sklearn():
    from hvamd import linear_probe
    with pytest.raises(ValueError, match="cannot be greater than the number of members in each class"):
        linear_probe.stratified_folds(np.array([0, 0, 1, 1, 2, 2, 0, 1]), 5)
    with pytest.warns(UserWarning, match="least populated class in y has only 1 members"):
        linear_probe.stratified_folds(np.array([3, 0, 0, 1, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0]), 5)
    with pytest.raises(ValueError, match="greater than the number of samples"):
        linear_probe.stratified_folds(np.array([0, 1, 0]), 5)


def test_scaler_restatement_zero_variance():
    mean, scale = ref.scaler(np.array([[1.0, 5.0], [3.0, 5.0]]))
    assert mean.tolist() == [2.0, 5.0] and scale.tolist() == [1.0, 1.0]


def test_restatement_gradient_is_the_losss_derivative():
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((20, 3)), rng.integers(0, 2, 20)
    W, b = rng.standard_normal((2, 3)), rng.standard_normal(2)
    target, alpha = np.arange(2), np.array([0.1, 1.0])
    dW, db, loss, _ = ref.loss_grad(X, y, W, b, target, alpha)
    h = 1e-6
    W2 = W.copy()
    W2[1, 2] += h
    assert abs((ref.loss_grad(X, y, W2, b, target, alpha)[2][1] - loss[1]) / h - dW[1, 2]) < 1e-5
    b2 = b.copy()
    b2[0] += h
    assert abs((ref.loss_grad(X, y, W, b2, target, alpha)[2][0] - loss[0]) / h - db[0]) < 1e-5


# --------------------------------------------------------------------------- C ABI
P = ctypes.c_void_p
ENTRY = ("hvk_lp_moments", "hvk_lp_standardize", "hvk_lp_loss_grad", "hvk_lp_decision", "hvk_lp_step")


def _args(name, **over):
    a = {
        "hvk_lp_moments": dict(x=P(0x1000), B=4, D=8, ld=8, sum=P(0x2000), sumsq=P(0x3000), count=None, stream=None),
        "hvk_lp_standardize": dict(x=P(0x1000), B=4, D=8, ld=8, sum=P(0x2000), sumsq=P(0x3000), n=4, out=P(0x4000),
                                   mean=P(0x5000), inv_std=P(0x6000), stream=None),
        "hvk_lp_loss_grad": dict(xs=P(0x1000), N=4, D=8, labels=P(0x2000), fold=None, skip_fold=-1, W=P(0x3000),
                                 b=P(0x4000), target=P(0x5000), alpha=P(0x6000), R=3, dW=P(0x7000), db=P(0x8000),
                                 loss=P(0x9000), workspace=P(0x10000), workspace_bytes=1 << 30, stream=None),
        "hvk_lp_decision": dict(xs=P(0x1000), B=4, D=8, W=P(0x3000), b=P(0x4000), R=3, out=P(0x7000), stream=None),
        "hvk_lp_step": dict(W=P(0x1000), b=P(0x2000), Yw=P(0x3000), Yb=P(0x4000), dW=P(0x5000), db=P(0x6000),
                            t=P(0x7000), frozen=None, R=3, D=8, step=0.5, tol=1e-4, gmax=P(0x8000),
                            converged=P(0x9000), stream=None),
    }[name]
    assert set(over) <= set(a), (name, over)
    a.update(over)
    return list(a.values())


def test_symbols_exported_and_bound():
    from hvamd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY + ("hvk_lp_loss_grad_workspace",):
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        assert len(_lib.SIGNATURES[name][1]) == (3 if name.endswith("workspace") else len(_args(name)))
    assert _lib.ABI_VERSION >= 19 and _lib.load().hvk_abi_version() == _lib.ABI_VERSION


_NULLS = {"hvk_lp_moments": ("x", "sum", "sumsq"),
          "hvk_lp_standardize": ("x", "sum", "sumsq", "out", "mean", "inv_std"),
          "hvk_lp_loss_grad": ("xs", "labels", "W", "b", "target", "alpha", "dW", "db", "loss"),
          "hvk_lp_decision": ("xs", "W", "b", "out"),
          "hvk_lp_step": ("W", "b", "Yw", "Yb", "dW", "db", "t", "gmax", "converged")}
BAD = [(n, {k: None}, b"null") for n, ks in _NULLS.items() for k in ks]
BAD += [(n, dict(D=0), b"shape") for n in ENTRY]
BAD += [("hvk_lp_moments", dict(B=-1), b"shape"), ("hvk_lp_moments", dict(ld=7), b"shape"),
        ("hvk_lp_standardize", dict(ld=7), b"shape"), ("hvk_lp_standardize", dict(n=0), b"shape"),
        ("hvk_lp_loss_grad", dict(N=0), b"shape"), ("hvk_lp_loss_grad", dict(R=0), b"shape"),
        ("hvk_lp_loss_grad", dict(workspace=None), b"workspace"),
        ("hvk_lp_loss_grad", dict(workspace_bytes=64), b"workspace"),
        ("hvk_lp_loss_grad", dict(workspace=P(0x10004)), b"workspace"),
        ("hvk_lp_decision", dict(B=-1), b"shape"), ("hvk_lp_decision", dict(R=0), b"shape"),
        ("hvk_lp_step", dict(R=0), b"shape"), ("hvk_lp_step", dict(step=0.0), b"step"),
        ("hvk_lp_step", dict(tol=-1.0), b"tol")]


@pytest.mark.parametrize("name,over,word", BAD, ids=[f"{b[0][7:]}-{'-'.join(b[1])}-{i}" for i, b in enumerate(BAD)])
def test_invalid_arguments_refused_before_any_launch(name, over, word):
    from hvamd import _lib
    lib = _lib.load()
    assert getattr(lib, name)(*_args(name, **over)) == HVK_EINVAL
    msg = lib.hvk_last_error_string()
    assert name.encode() in msg and word in msg, msg


def test_empty_batch_is_ok_without_a_launch():
    from hvamd import _lib
    lib = _lib.load()
    assert lib.hvk_lp_moments(*_args("hvk_lp_moments", B=0)) == HVK_OK
    assert lib.hvk_lp_decision(*_args("hvk_lp_decision", B=0)) == HVK_OK
    assert lib.hvk_lp_loss_grad(*_args("hvk_lp_loss_grad", R=1 << 20)) == 2  # HVK_EUNSUPPORTED


def test_workspace_arithmetic():
    """One chunk of residuals [CH, Rp], S slabs [Rp, Dp], two float64 partials per (row tile,
    class), two float64 sums per class and the row count; every part rounded up to 256 bytes."""
    from hvamd import _lib
    lib = _lib.load()
    r256 = lambda v: (v + 255) // 256 * 256  # noqa: E731
    # N 67, D 100, R 37: CH 128, Rp 64, Dp 128, 2 tiles -> 4 row splits of one 32-row stage
    want = r256(128 * 64 * 4) + r256(4 * 64 * 128 * 4) + 2 * r256(2 * 64 * 8) + 2 * r256(64 * 8) + 256
    assert lib.hvk_lp_loss_grad_workspace(67, 100, 37) == want
    assert lib.hvk_lp_loss_grad_workspace(0, 100, 37) == 0 and lib.hvk_lp_loss_grad_workspace(67, 100, 1 << 20) == 0
    assert lib.hvk_lp_loss_grad_workspace(8192, 8, 3) == lib.hvk_lp_loss_grad_workspace(1 << 30, 8, 3)


# --------------------------------------------------------------------------- Python surface
def test_wrappers_refuse_bad_arguments():
    import hvamd.ops as ops
    x, W = torch.zeros(4, 8), torch.zeros(3, 8)
    y, b = torch.zeros(4, dtype=torch.int64), torch.zeros(3)
    tg, al = torch.arange(3, dtype=torch.int32), torch.zeros(3)
    s = torch.zeros(8, dtype=torch.float64)
    with pytest.raises(ValueError, match="float32"):
        ops.lp_moments(x.double(), s, s.clone())
    with pytest.raises(ValueError, match=r"\[B, D\]"):
        ops.lp_moments(x[0], s, s.clone())
    with pytest.raises(ValueError, match="float64"):
        ops.lp_moments(x, s.float(), s.clone())
    with pytest.raises(ValueError, match="float64"):
        ops.lp_standardize(x, s[:4], s, 4)
    with pytest.raises(ValueError, match="fit the scaler"):
        ops.lp_standardize(x, s, s.clone(), 0)
    with pytest.raises(ValueError, match="float32"):
        ops.lp_loss_grad(x.half(), y, W, b, tg, al)
    with pytest.raises(ValueError, match="contiguous"):
        ops.lp_loss_grad(torch.zeros(8, 4).t(), y, W, b, tg, al)
    with pytest.raises(ValueError, match="int64"):
        ops.lp_loss_grad(x, y.int(), W, b, tg, al)
    with pytest.raises(ValueError, match="must be"):
        ops.lp_loss_grad(x, y, torch.zeros(3, 7), b, tg, al)
    with pytest.raises(ValueError, match="target"):
        ops.lp_loss_grad(x, y, W, b, tg.long(), al)
    with pytest.raises(ValueError, match="fold"):
        ops.lp_loss_grad(x, y, W, b, tg, al, fold=torch.zeros(4, dtype=torch.int32), skip_fold=0)
    with pytest.raises(ValueError, match=r"labels outside \[0, 3\)"):
        ops.lp_loss_grad(x, torch.tensor([0, 1, 3, 2]), W, b, tg, al)
    with pytest.raises(ValueError, match=r"labels outside \[0, 3\)"):
        ops.lp_loss_grad(x, torch.tensor([0, -1, 2, 2]), W, b, tg, al)
    with pytest.raises(ValueError, match="does not fit"):
        ops.lp_step(W, b, torch.zeros(3, 7), b, W, b, b, 0.5, 1e-4, b, torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="step"):
        ops.lp_step(W, b, W, b, W, b, b, 0.0, 1e-4, b, torch.zeros(3, dtype=torch.uint8))
    # well-formed CPU tensors get as far as _lib.ptr, which refuses them
    for fn in (lambda: ops.lp_moments(x, s, s.clone()), lambda: ops.lp_standardize(x, s, s.clone(), 4),
               lambda: ops.lp_loss_grad(x, y, W, b, tg, al), lambda: ops.lp_decision(x, W, b),
               lambda: ops.lp_step(W, b, W.clone(), b, W, b, b, 0.5, 1e-4, b, torch.zeros(3, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn()


def test_estimators_refuse_bad_arguments():
    from hvamd import linear_probe
    clf = linear_probe.LogisticOvR(n_classes=3)
    with pytest.raises(ValueError, match="labels outside"):
        clf.fit(torch.zeros(4, 8), torch.tensor([0, 1, 2, 3]))
    with pytest.raises(ValueError, match="integer"):
        clf.fit(torch.zeros(4, 8), torch.zeros(4))
    with pytest.raises(ValueError, match="go together"):
        clf.fit(torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64), fold=torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="not fitted"):
        clf.predict(torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="not fitted"):
        linear_probe.StandardScaler().transform(torch.zeros(4, 8))
    with pytest.raises(ValueError, match="alpha"):
        linear_probe.LogisticOvR(alpha=-1.0).fit(torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64))


def test_evaluate_rejects_other_variants():
    import hvamd
    from hvamd import configs, linear_probe
    assert hvamd.linear_probe is linear_probe
    cfg = configs.Config()
    for variant in ("full-tuning", "simpleshot"):
        cfg.model.variant = variant
        with pytest.raises(AssertionError, match=variant):
            linear_probe.evaluate(cfg, None, [], [])
    cfg.model.variant = "linear-probe"
    with pytest.raises(ValueError, match="FeatureOnlyModel"):
        linear_probe.evaluate(cfg, torch.nn.Identity(), [], [])
