"""Write profiles/wmsa/baseline_blocks.txt: the honest-bf16 baseline of every case of
tests/test_gpu_wmsa_blocks.py -- tests/wmsa_ref.py::core(round_ops=True) against
core(round_ops=False), the worst normalised error per class.  CPU only, from the reference alone;
the GPU test recomputes the same figures at run time and bounds the kernels at 2 x them.

    python tools/wmsa_baseline_blocks.py [output file]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import wmsa_ref as R  # noqa: E402

HEADER = """\
W-MSA block baseline: float64 math with the kernels' bf16 operand roundings (tests/wmsa_ref.py,
round_ops=True, list of operands in its docstring) against plain float64, per case the worst unit
of each class.  Units and sizes: out / dq / dk / dv one (image, window, head) block over the
float64 block's norm; dbias one table entry over sum |dS|; dscale one head over sum |dS cos|;
dq_bias one channel over sum |dq|.  Inputs: the _inputs recipe of tests/test_gpu_wmsa.py, seeds
%d (qkv, table, scale) and %d (gout).  Written by tools/wmsa_baseline_blocks.py.
""" % (R.SEED_IN, R.SEED_GOUT)


def main(path):
    lines, zeros = [HEADER], []
    for group, geom, form in R.BLOCK_CASES:
        lines.append(f"{R.case_id(group, geom)}  (backward form {form})")
        for name, v, where in R.baseline_rows(group, geom, form):
            lines.append(f"  {name:<8s} {v:.3e}   {where}")
            if v == 0:
                zeros.append((R.case_id(group, geom), name))
        lines.append("")
    lines.append("classes with a baseline of 0: " + (", ".join(f"{c} {n}" for c, n in zeros) if zeros else "none"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "wmsa", "baseline_blocks.txt"))
