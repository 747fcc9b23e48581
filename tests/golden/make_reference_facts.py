"""Record, once, the facts of the reference project that the CPU suite checks, so that the suite needs nothing outside
the repository: tests/golden/reference_facts.json.

    python tests/golden/make_reference_facts.py <reference checkout>

Needs oracle/_ref/libref_matrix.so (`make -C oracle ref REF=<reference checkout>/code/MPI`): the reference's own
Matrix-Market reader, whose output on the fixture and on tests/test_oracle.py's MTX_CASES is stored here.
  - lap2D_5pt_n100.mtx : sha256 and size of the reference's copy of the file (tests/golden/ holds a regenerated one)
  - plots_ipynb        : the ALPHAS table, ITEMS and the BETAS slice of the notebook's first code cell
  - ref_reader         : what Matrix::read (code/MPI/matrix.cc) makes of each file: the dense matrix for the small
                         cases, shape, non-zero count and sha256 of the row-major float64 bytes for the fixture
"""
import hashlib
import importlib.util
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def dense_digest(A):
    import numpy as np
    A = np.ascontiguousarray(A, dtype=np.float64)
    return {"shape": list(A.shape), "nnz": int(np.count_nonzero(A)), "sha256": hashlib.sha256(A.tobytes()).hexdigest()}


def main(ref_root):
    sys.path.insert(0, ROOT)
    from oracle import oracle
    assert oracle.ref_available(), "build oracle/_ref first (make -C oracle ref)"
    spec = importlib.util.spec_from_file_location("test_oracle", os.path.join(ROOT, "tests", "test_oracle.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)

    mtx = open(os.path.join(ref_root, "code", "MPI", "lap2D_5pt_n100.mtx"), "rb").read()
    cells = json.load(open(os.path.join(ref_root, "plots.ipynb")))["cells"]
    src = "".join("".join(c["source"]) for c in cells if c["cell_type"] == "code")
    table = re.search(r"ALPHAS\s*=\s*\{(.*?)\}", src, re.S).group(1)
    alphas = [[int(k), 1.0 - float(v)] for k, v in re.findall(r"(\d+)\s*:\s*1-([0-9.]+)", table)]
    items = int(re.search(r"ITEMS\s*=\s*(\d+)", src).group(1))
    betas = int(re.search(r"BETAS\s*=\s*list\(ALPHAS\.values\(\)\)\[(\d+):\]", src).group(1))

    reader = {"lap2D_5pt_n100.mtx": dense_digest(oracle.ref_read_mtx_dense(os.path.join(HERE, "lap2D_5pt_n100.mtx")))}
    with tempfile.TemporaryDirectory() as d:
        for name, text in t.MTX_CASES.items():
            f = os.path.join(d, name)
            with open(f, "w") as fh:
                fh.write(text)
            reader[name] = {"dense": oracle.ref_read_mtx_dense(f).tolist()}

    facts = {"lap2D_5pt_n100.mtx": {"bytes": len(mtx), "sha256": hashlib.sha256(mtx).hexdigest()},
             "plots_ipynb": {"alphas": alphas, "items": items, "betas_slice_start": betas},
             "ref_reader": reader}
    with open(os.path.join(HERE, "reference_facts.json"), "w") as f:
        json.dump(facts, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
