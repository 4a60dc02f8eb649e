"""Writes tests/golden/ssl_step.npz: the fp64 oracle's outputs (tests/ssl_oracle.py) for the data-dependent init, one classifier step and
one generator step of the semi-supervised CT classifier at reduced widths (ssl_oracle.small_cfg, seed 5): the init's weight scales and
biases, the step's scalars and ct_i, every gradient (stored fp32).  tests/test_ssl_host.py pins the oracle to the file,
tests/test_gpu_ssl.py the product.  Run from the repository root:  python tests/golden/make_ssl_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def compute():
    import ctgan_amd.ct_mnist as M
    from tests import ssl_oracle as O
    O.small_cfg()
    try:
        return O.oracle_golden(M.cfg)
    finally:
        M.configure()


if __name__ == '__main__':
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ssl_step.npz')
    np.savez_compressed(out, **compute())
    print('wrote', out, os.path.getsize(out), 'bytes')
