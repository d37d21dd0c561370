"""Write tests/golden/dgrad_column_classes.json: sha256 of the bytes sf_conv_dgrad produces for the golden cases of
tests/test_gpu_dgrad_column_classes.py (seeded inputs, with and without the ReLU mask).  Run on a GPU with the commit
checked out whose results are to be pinned: the file in the tree was written by the last commit whose conv2 data gradient
still multiplied the zero tap columns of the image border.  python tools/gen_golden_dgrad_classes.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_gpu_dgrad_column_classes as T  # noqa: E402


def main():
    out = {}
    for geom, n in T.GOLDEN_CASES:
        for mode in T.MODES:
            name, din, intact = T.launch(geom, n, mode)
            assert intact and name.startswith("k_dgrad_quadrow"), (name, intact)
            out[f"{T.case_id(geom, n)}-{mode}"] = T.digest(din)
            print(f"{T.case_id(geom, n)}-{mode} {name} {out[f'{T.case_id(geom, n)}-{mode}']}", flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN, "w") as f:
        json.dump({"what": "sha256 of din (f32 NHWC bytes) per case of tests/test_gpu_dgrad_column_classes.py", "sha256": out},
                  f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
