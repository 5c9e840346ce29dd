"""Regenerates tests/golden/downsample_golden.npz from the REAL reference.  Run by hand, never by a test:

    python tests/golden/make_downsample_golden.py <reference root> [scratch directory]

Compiles the reference's ops/{fps,cluster}.cpp and ops/cpu/{fps,cluster}_kernel.cpp where they lie (the g++ line of
tests/golden/make_spatial_golden.py) into a scratch directory, loads the library and records what its CPU kernels return.
Only inputs and index outputs are stored.  Must not import pyg_lib_amd: both libraries define the `pyg` operator schemas."""
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
from tests import _downsample_ref as ref   # noqa: E402
import downsample_cases as cases   # noqa: E402


def build(ref_root, scratch):
    tdir = osp.dirname(torch.__file__)
    abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)
    srcs = ['ops/fps', 'ops/cpu/fps_kernel', 'ops/cluster', 'ops/cpu/cluster_kernel']
    objs = []
    for s in srcs:
        o = osp.join(scratch, s.replace('/', '_') + '.o')
        subprocess.check_call(['g++', '-std=c++20', '-O2', '-fPIC', '-fopenmp', f'-D_GLIBCXX_USE_CXX11_ABI={abi}', f'-I{ref_root}',
                               f'-I{tdir}/include', f'-I{tdir}/include/torch/csrc/api/include', '-Wno-deprecated-declarations',
                               '-c', osp.join(ref_root, 'pyg_lib', 'csrc', s + '.cpp'), '-o', o])
        objs.append(o)
    lib = osp.join(scratch, 'libpyg_ref_downsample.so')
    subprocess.check_call(['g++', '-shared', '-fopenmp'] + objs + ['-o', lib, f'-L{tdir}/lib', '-ltorch', '-ltorch_cpu', '-lc10',
                                                                 f'-Wl,-rpath,{tdir}/lib'])
    return lib


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ['REF']   # the pyg-lib source tree
    scratch = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix='downsample_ref_')
    os.makedirs(scratch, exist_ok=True)
    torch.ops.load_library(build(ref_root, scratch))
    out = {}
    for key, D, name in cases.fps_clouds():
        src, ptr, seed = ref.tie_free_cloud(cases.FPS_SIZES, D, cases.FPS_DTYPES[name], ratio=1.0, seed=0)
        print(key, 'seed', seed)
        out[f'{key}/src'] = src.numpy()
        for ratio in cases.FPS_RATIOS:
            got = torch.ops.pyg.fps(src, ptr, ratio, False)
            assert torch.equal(got, ref.fps(src, ptr, ratio)), (key, ratio)
            out[f'{key}/ratio{ratio}'] = got.numpy()
    for key, N, D, name in cases.grid_clouds():
        pos, size, start, end = cases.grid_inputs(N, D, name)
        free = torch.ops.pyg.grid_cluster(pos, size, None, None)
        bound = torch.ops.pyg.grid_cluster(pos, size, start, end)
        assert torch.equal(free, ref.grid_cluster_for(pos, size)) and torch.equal(bound, ref.grid_cluster_for(pos, size, start, end)), key
        out[f'{key}/free'], out[f'{key}/bound'] = free.numpy(), bound.numpy()
    path = osp.join(HERE, 'downsample_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, osp.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
