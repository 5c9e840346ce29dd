"""Regenerates tests/golden/graclus_golden.npz from the REAL reference.  Run by hand, never by a test:

    python tests/golden/make_graclus_golden.py <reference root> [scratch directory]

Compiles the reference's ops/graclus.cpp and ops/cpu/graclus_kernel.cpp where they lie (the g++ line of
tests/golden/make_downsample_golden.py) into a scratch directory, loads the library and records what its CPU kernel returns
under torch.manual_seed(seed), with the permutation torch.randperm draws under that seed.  Only inputs and index outputs are
stored.  Must not import pyg_lib_amd: both libraries define the `pyg` operator schemas."""
import os
import os.path as osp
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, osp.dirname(osp.dirname(HERE)))
sys.path.insert(0, HERE)
from tests import _graclus_ref as ref   # noqa: E402
import graclus_cases as cases   # noqa: E402


def build(ref_root, scratch):
    tdir = osp.dirname(torch.__file__)
    abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)
    objs = []
    for s in ['ops/graclus', 'ops/cpu/graclus_kernel']:
        o = osp.join(scratch, s.replace('/', '_') + '.o')
        subprocess.check_call(['g++', '-std=c++20', '-O2', '-fPIC', '-fopenmp', f'-D_GLIBCXX_USE_CXX11_ABI={abi}', f'-I{ref_root}',
                               f'-I{tdir}/include', f'-I{tdir}/include/torch/csrc/api/include', '-Wno-deprecated-declarations',
                               '-c', osp.join(ref_root, 'pyg_lib', 'csrc', s + '.cpp'), '-o', o])
        objs.append(o)
    lib = osp.join(scratch, 'libpyg_ref_graclus.so')
    subprocess.check_call(['g++', '-shared', '-fopenmp'] + objs + ['-o', lib, f'-L{tdir}/lib', '-ltorch', '-ltorch_cpu', '-lc10',
                                                                 f'-Wl,-rpath,{tdir}/lib'])
    return lib


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ['REF']   # the pyg-lib source tree
    scratch = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix='graclus_ref_')
    os.makedirs(scratch, exist_ok=True)
    torch.ops.load_library(build(ref_root, scratch))
    out = {}
    for key, family, kind, dtype_name, seed in cases.CASES:
        rowptr, col = ref.FAMILIES[family]()
        N = rowptr.numel() - 1
        weight = ref.weights(kind, col.numel(), cases.dtype_of(dtype_name) or torch.float32, seed)
        torch.manual_seed(seed)
        perm = torch.randperm(N)
        torch.manual_seed(seed)
        got = torch.ops.pyg.graclus_cluster(rowptr, col, weight)
        assert torch.equal(got, ref.sequential(rowptr, col, weight, perm)), key
        assert torch.equal(got, ref.rounds(rowptr, col, weight, perm)[0]), key
        out[f'{key}/rowptr'], out[f'{key}/col'] = rowptr.numpy(), col.numpy()
        if weight is not None:
            out[f'{key}/weight'] = cases.to_numpy(weight)
        out[f'{key}/seed'], out[f'{key}/perm'], out[f'{key}/out'] = np.int64(seed), perm.numpy(), got.numpy()
        print(key, 'N', N, 'E', col.numel(), 'clusters', int(got.unique().numel()))
    path = osp.join(HERE, 'graclus_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, osp.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
