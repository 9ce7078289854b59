"""Generates tests/golden/detect.npz: the data the source-detection tests need, taken from the reference's sample data
(run once where the reference's sources are; the tests read only the .npz).

Contents:
  field2_r, field3_r     the r band (index 2) of data/dc2_imgs/field/field_img_2.npy and field_img_3.npy, float32 (the
                         fields are float32-exact)
  truth2, truth3         their truth catalogs (gal_coordinates_complete_truth_catalog_{2,3}.npy): (x, y) in tile pixels
  center2, center3       the field centres (field_center_{2,3}.npy), (cx, cy) in tile pixels
  ref_filter             the 7 x 7 filter table of the reference's detect_objects, read as data
A truth galaxy (x, y) sits at field row y - cy + F // 2, column x - cx + F // 2.

Usage:  python tests/golden/make_detect_golden.py /path/to/debvader/src/debvader
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _filter_table(src):
    """the literal assigned to filter_kernel in the reference's detection.py, parsed as data (never executed)"""
    tree = ast.parse(open(src).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "filter_kernel" for t in node.targets):
            return np.array(ast.literal_eval(node.value.args[0]), dtype=np.float64)
    raise RuntimeError("no filter_kernel table in " + src)


def main(ref):
    d = os.path.join(ref, "data", "dc2_imgs", "field")
    out = {}
    for k in (2, 3):
        r = np.load(os.path.join(d, f"field_img_{k}.npy"))[0, :, :, 2]
        assert np.array_equal(r.astype(np.float32).astype(np.float64), r), "the r band is not float32-exact"
        out[f"field{k}_r"] = r.astype(np.float32)
        out[f"truth{k}"] = np.asarray(np.load(os.path.join(d, f"gal_coordinates_complete_truth_catalog_{k}.npy"),
                                              allow_pickle=True), dtype=np.float64)
        out[f"center{k}"] = np.asarray(np.load(os.path.join(d, f"field_center_{k}.npy"), allow_pickle=True),
                                       dtype=np.float64)
    out["ref_filter"] = _filter_table(os.path.join(ref, "detect", "detection.py"))
    np.savez_compressed(os.path.join(HERE, "detect.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
