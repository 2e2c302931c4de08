#!/usr/bin/env python3
"""Record tests/golden/headline_rows_bits.npz: the outputs of the batch of tests/test_headline_rows_bits.py, part (a),
from the library that is built in the tree (or named by PP_TOAS_LIB).

Run ONCE, on a GPU, from the build of the commit BEFORE a change that has to leave the headline row loop's bits alone:

    python tests/golden/make_golden_headline_rows_bits.py [OUT.npz]

The file is a record of what that build computed.  It is not regenerated from the code under test: the script
refuses to overwrite it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from pulseportraiture_amd.engine import Engine
    from tests import test_headline_rows_bits as t
    out = sys.argv[1] if len(sys.argv) > 1 else t.FIXTURE
    if os.path.exists(out):
        sys.exit("%s exists: it is a record of an earlier build and is not regenerated" % out)
    e = Engine(0)
    r, eps = t.headline_rows_batch(e)
    again, _ = t.headline_rows_batch(e)
    e.close()
    for k in t.BITWISE:      # (what is recorded does not move from run to run)
        np.testing.assert_array_equal(r[k], again[k], err_msg=k)
    print("harm_eps %.3e  return_code %s  npass %s  nfeval %s" %
          (eps, sorted(set(r["return_code"].tolist())), sorted(set(r["npass"].tolist())), sorted(set(r["nfeval"].tolist()))))
    np.savez(out, harm_eps=np.float64(eps), **{k: r[k] for k in t.BITWISE})
    print("wrote", out)


if __name__ == "__main__":
    main()
