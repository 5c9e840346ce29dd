"""Regenerates tests/golden/spatial_golden.npz from the REAL reference.  Run by hand, never by a test:

    python tests/golden/make_spatial_golden.py [reference root] [scratch directory]

Compiles the reference's ops/{knn,radius,nearest}.cpp and ops/cpu/{knn,radius,nearest}_kernel.cpp where they lie (the g++ line
of oracle/build_ref.sh; nanoflann is vendored in the reference) into a scratch directory, loads the library and records what
its CPU kernels return.  Only inputs and index outputs are stored.  Must not import pyg_lib_amd: both libraries define the
`pyg` operator schemas."""
import os
import os.path as osp
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, osp.dirname(HERE))
sys.path.insert(0, HERE)
import _spatial_ref as ref   # noqa: E402
import spatial_cases as cases   # noqa: E402


def build(ref_root, scratch):
    tdir = osp.dirname(torch.__file__)
    abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)
    srcs = [f'ops/{n}' for n in ('knn', 'radius', 'nearest')] + [f'ops/cpu/{n}_kernel' for n in ('knn', 'radius', 'nearest')]
    objs = []
    for s in srcs:
        o = osp.join(scratch, s.replace('/', '_') + '.o')
        subprocess.check_call(['g++', '-std=c++20', '-O2', '-fPIC', '-fopenmp', f'-D_GLIBCXX_USE_CXX11_ABI={abi}', f'-I{ref_root}',
                               f'-I{tdir}/include', f'-I{tdir}/include/torch/csrc/api/include', '-Wno-deprecated-declarations',
                               '-c', osp.join(ref_root, 'pyg_lib', 'csrc', s + '.cpp'), '-o', o])
        objs.append(o)
    lib = osp.join(scratch, 'libpyg_ref_spatial.so')
    subprocess.check_call(['g++', '-shared', '-fopenmp'] + objs + ['-o', lib, f'-L{tdir}/lib', '-ltorch', '-ltorch_cpu', '-lc10',
                                                                 f'-Wl,-rpath,{tdir}/lib'])
    return lib


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('REF', '/root/reference')
    scratch = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix='spatial_ref_')
    os.makedirs(scratch, exist_ok=True)
    torch.ops.load_library(build(ref_root, scratch))
    out = {}
    for key, D, name in cases.clouds():
        dtype = cases.DTYPES[name]
        x, y, ptr_x, ptr_y, seed = ref.tie_free_clouds(cases.X_SIZES, cases.Y_SIZES, D, dtype, max(cases.KS), seed=0,
                                                       radii=cases.radii(D))
        print(key, 'seed', seed)
        out[f'{key}/x'], out[f'{key}/y'] = x.numpy(), y.numpy()
        for k in cases.KS:
            got = torch.ops.pyg.knn(x, y, ptr_x, ptr_y, k, False, 1)
            assert torch.equal(got, ref.knn(x, y, k, ptr_x, ptr_y)), (key, k)   # (nearest first per query: no sorting)
            out[f'{key}/knn{k}'] = got.numpy()
        for r in cases.radii(D):
            got = ref.sort_pairs(torch.ops.pyg.radius(x, y, ptr_x, ptr_y, r, cases.MAX_NEIGHBORS, 1, False))
            out[f'{key}/radius{r}'] = got.numpy()
        out[f'{key}/nearest'] = torch.ops.pyg.nearest(x, y, ptr_x, ptr_y).numpy()
    np.savez_compressed(osp.join(HERE, 'spatial_golden.npz'), **out)
    print('wrote', osp.join(HERE, 'spatial_golden.npz'), osp.getsize(osp.join(HERE, 'spatial_golden.npz')), 'bytes')


if __name__ == '__main__':
    main()
