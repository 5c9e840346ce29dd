"""Reader for tests/golden/special_golden.part*.npz (outputs of the REAL reference CPU kernels on non-finite values, signed
zeros, the types' limits and denormals, recorded by tests/golden/make_special_golden.py through oracle/_ref), and THE
comparison rule of the special-value tests (`same_bits`)."""
import numpy as np

from tests.golden import parts

_D = None
TAGS = ('f32', 'f64', 'bf16', 'f16')
_UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def data():
    global _D
    if _D is None:
        _D = parts.load('special_golden')
    return _D


def names(prefix):
    return [str(n) for n in data()['__cases__'] if str(n).startswith(prefix)]


def _get(key):
    d = data()
    return d[key] if key in d else None


def case(name):
    """'scatter_f32_fresh_sum' | 'coo_bf16_out_min' | 'csr_f16_out_mean' | 'gathercoo_f64' | 'gathercsr_f32' | 'softmax_f32'
    -> dict of numpy arrays (bf16 as uint16 bit patterns, flagged by 'bf16')."""
    f = name.split('_')
    fam, tag = f[0], f[1]
    out = {'name': name, 'family': fam, 'tag': tag, 'bf16': tag == 'bf16'}
    if fam == 'softmax':
        for k in ('src', 'ptr', 'res', 'out_grad', 'in_grad'):
            out[k] = _get(f'{name}_{k}')
        return out
    out['res'], out['arg'] = _get(name + '_res'), _get(name + '_arg')
    out['out0'] = _get(f'{tag}_out0')
    out['indptr'] = _get(f'{tag}_indptr')
    out['N'] = out['out0'].shape[0]
    if fam in ('gathercoo', 'gathercsr'):
        out['src'], out['index'] = out['out0'], _get(f'{tag}_index_sorted')
        out['E'] = out['index'].shape[0]
        return out
    out['mode'], out['op'] = f[2], f[3]
    which = 'unsorted' if fam == 'scatter' else 'sorted'
    out['src'], out['index'] = _get(f'{tag}_src_{which}'), _get(f'{tag}_index_{which}')
    if out['mode'] == 'fresh':
        out['out0'] = None
    return out


def bits(a):
    """The bit patterns of a floating (or already unsigned) numpy array."""
    a = np.ascontiguousarray(a)
    return a if a.dtype.kind == 'u' else a.view(_UINT[a.dtype.itemsize])


def as_float(a, bf16=False):
    """float64 values of an array (`bf16`: uint16 bit patterns)."""
    a = np.ascontiguousarray(a)
    if bf16:
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return a.astype(np.float64)


def same_bits(got, ref, bf16=False, nan_bits=False, what=''):
    """The comparison rule of the special-value tests: NaN exactly where the reference has NaN (sign and payload free,
    unless `nan_bits`: plain copies keep them), every other element bit for bit -- the sign of a zero and of an Inf counts."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    gn, rn = np.isnan(as_float(got, bf16)), np.isnan(as_float(ref, bf16))
    if nan_bits:
        gn, rn = np.zeros_like(gn), np.zeros_like(rn)
    assert np.array_equal(gn, rn), f'{what}: NaN at {np.argwhere(gn != rn)[:8].tolist()} (got / reference differ)'
    gb, rb = bits(got), bits(ref)
    bad = (gb != rb) & ~rn
    if bad.any():
        at = np.argwhere(bad)[:8]
        show = [(tuple(i), float(as_float(got, bf16)[tuple(i)]), float(as_float(ref, bf16)[tuple(i)]), hex(int(gb[tuple(i)])),
                 hex(int(rb[tuple(i)]))) for i in at]
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements differ: (index, got, want, got bits, want bits) {show}')
