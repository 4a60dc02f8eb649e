"""Writes tests/golden/ssl_cifar_te_step.npz: the fp64 oracle's outputs (tests/ssl_cifar_te_oracle.py) for the data-dependent init,
one classifier step against non-zero target tables and one generator step of the temporal-ensembling CT classifier at reduced
sizes (ssl_cifar_te_oracle.small_cfg, seed 5): the init's g and b, the steps' scalars, the prediction rows the classifier step
files, and the gradients of the parameters of at most 512 elements (stored fp32; the file stays small).
tests/test_ssl_cifar_te_host.py pins the oracle to the file, tests/test_gpu_ssl_cifar_te.py the product.  Run from the repository
root:  python tests/golden/make_ssl_cifar_te_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def compute():
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.ct_cifar_te as T
    from tests import ssl_cifar_te_oracle as O
    O.small_cfg()
    try:
        return O.oracle_golden(T.cfg)
    finally:
        T.configure(); M.configure()


if __name__ == '__main__':
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ssl_cifar_te_step.npz')
    np.savez_compressed(out, **compute())
    print('wrote', out, os.path.getsize(out), 'bytes')
