"""Regenerates tests/golden/spline_golden.npz from the REAL reference.  Run by hand, never by a test:

    python tests/golden/make_spline_golden.py <reference root> [scratch directory]

Compiles the reference's ops/spline.cpp, ops/cpu/spline_kernel.cpp and ops/autograd/spline_kernel.cpp where they lie (the g++
line of tests/golden/make_downsample_golden.py) into a scratch directory, loads the library and records the inputs and what
its six CPU operators return.  Must not import pyg_lib_amd: both libraries define the `pyg` operator schemas."""
import os
import os.path as osp
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, HERE)
import spline_cases as cases   # noqa: E402


def build(ref_root, scratch):
    tdir = osp.dirname(torch.__file__)
    abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)
    srcs = ['ops/spline', 'ops/cpu/spline_kernel', 'ops/autograd/spline_kernel']
    objs = []
    for s in srcs:
        o = osp.join(scratch, s.replace('/', '_') + '.o')
        subprocess.check_call(['g++', '-std=c++20', '-O2', '-fPIC', '-fopenmp', f'-D_GLIBCXX_USE_CXX11_ABI={abi}', f'-I{ref_root}',
                               f'-I{tdir}/include', f'-I{tdir}/include/torch/csrc/api/include', '-Wno-deprecated-declarations',
                               '-c', osp.join(ref_root, 'pyg_lib', 'csrc', s + '.cpp'), '-o', o])
        objs.append(o)
    lib = osp.join(scratch, 'libpyg_ref_spline.so')
    subprocess.check_call(['g++', '-shared', '-fopenmp'] + objs + ['-o', lib, f'-L{tdir}/lib', '-ltorch', '-ltorch_cpu', '-lc10',
                                                                 f'-Wl,-rpath,{tdir}/lib'])
    return lib


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ['REF']   # the pyg-lib source tree
    scratch = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix='spline_ref_')
    os.makedirs(scratch, exist_ok=True)
    torch.ops.load_library(build(ref_root, scratch))
    ops = torch.ops.pyg
    out = {}
    for key, degree, D, open_name, name in cases.basis_cases():
        pseudo, kernel_size, is_open, grad_basis = cases.basis_inputs(degree, D, open_name, name)
        basis, weight_index = ops.spline_basis(pseudo, kernel_size, is_open, degree)
        grad_pseudo = ops.spline_basis_backward(grad_basis, pseudo, kernel_size, is_open, degree)
        for field, t in dict(pseudo=pseudo, kernel_size=kernel_size, is_open=is_open, grad_basis=grad_basis, basis=basis,
                             weight_index=weight_index, grad_pseudo=grad_pseudo).items():
            out[f'{key}/{field}'] = cases.to_numpy(t)
    for key, shape, name in cases.weighting_cases():
        x, weight, basis, weight_index, grad_out = cases.weighting_inputs(shape, name)
        res = dict(x=x, weight=weight, basis=basis, weight_index=weight_index, grad_out=grad_out,
                   out=ops.spline_weighting(x, weight, basis, weight_index),
                   grad_x=ops.spline_weighting_backward_x(grad_out, weight, basis, weight_index),
                   grad_weight=ops.spline_weighting_backward_weight(grad_out, x, basis, weight_index, shape[2]),
                   grad_basis=ops.spline_weighting_backward_basis(grad_out, x, weight, weight_index))
        for field, t in res.items():
            out[f'{key}/{field}'] = cases.to_numpy(t)
    path = osp.join(HERE, 'spline_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, osp.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
