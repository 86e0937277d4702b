"""Generate the shape fixtures of ``shape_cases.py`` by running the REFERENCE model (build container only).

    python tests/golden/make_golden_shapes.py [case ...]

The same recipe as ``make_golden.py`` (reference built in place by oracle/ref_import.py, weights from detrng.fill_module_,
inputs from detrng.make_inputs with the case's joint count; inputs, output and the spt_view0 / fpt_in / fused taps stored, plus
out_x1 / out_x2 for head_kadkhod).  No weights are stored.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.make_golden import run_case      # noqa: E402
from tests.golden.shape_cases import SHAPE_CASES   # noqa: E402


def main(argv):
    want = set(argv)
    for case in SHAPE_CASES:
        if not want or case["name"] in want:
            run_case(case)


if __name__ == "__main__":
    main(sys.argv[1:])
