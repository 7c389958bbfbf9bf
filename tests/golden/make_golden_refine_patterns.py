"""
Writes tests/golden/refine_patterns.npz: for the operators of test_refine_host.random_operators whose exact rows are too
expensive to compute in every test run (test_refine_host.EXACT_ROWS_BUDGET), the zero pattern of the exact rows of
tests/refine_ref.py, with the knots they belong to.  Pure Python Fractions, about two minutes.

    python tests/golden/make_golden_refine_patterns.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import refine_ref                                   # noqa: E402
import test_refine_host as trh                      # noqa: E402
from bspy_amd import refinement                     # noqa: E402


def main():
    out = {}
    for trial, order, m, t, new in trh.random_operators():
        tbar = refinement.elevated_knots(t, order, m, new) if m else refinement.merged_knots(t, order, new)[0]
        if trh.exact_rows_cost(order, m, len(tbar) - order - m) <= trh.EXACT_ROWS_BUDGET:
            continue
        rows = refine_ref.refine_rows(t, order, tbar, m)
        assert all(row is not None for row in rows)
        out[f"{trial}/knots"], out[f"{trial}/new_knots"] = t, tbar
        out[f"{trial}/pattern"] = trh.dense_pattern(rows, len(t) - order)
        print(f"trial {trial}: order {order}, m {m}, {len(rows)} rows", flush=True)
    np.savez_compressed(os.path.join(HERE, "refine_patterns.npz"), **out)


if __name__ == "__main__":
    main()
