"""Fresh-process half of tests/test_mona_contract_gpu.py::test_spatial_per_pixel_kernel_bf16_at_widths_14_and_4: the launcher reads UIA_MONA_FAST once
per process, so the bf16 cases of widths 14 and 4 run here, with UIA_MONA_FAST=0 in this process's environment, on the per-pixel kernel, and are
judged without the matrix-core term of the bound.

    UIA_MONA_FAST=0 python mona_perpixel_driver.py        prints the checker's report; exit status 1 if a comparison failed
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    assert os.environ.get("UIA_MONA_FAST") == "0", "run with UIA_MONA_FAST=0"
    import helpers_reference as R
    import mona_reference as MR
    import test_mona_contract_gpu as T
    from uia_hip import _lib, ops
    ck = R.Checker()
    for case in MR.FAST4_CASES + MR.FAST14_CASES:
        T.check_spatial(_lib.lib(), ops, ck, case, fast_allowed=False)
    print(ck.report())
    return 0 if ck.ok() else 1


if __name__ == "__main__":
    sys.exit(main())
