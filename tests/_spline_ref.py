"""Float64 restatement of the spline_weighting family (include/pyg_hip.h, "spline_basis, spline_weighting"), for error bounds:
every function returns (value, sum of |terms|) per output element, both float64, so that a test can require
|got - value| <= gamma_n * sum|terms| of a sequential sum of n terms (gamma_n = n u / (1 - n u)).  Inputs of any floating
dtype are widened exactly."""
import torch

CHUNK_EDGES = 64   # rows handled at a time: bounds the [edges, S, M_in, M_out] temporaries


def gamma(n, u):
    return n * u / (1.0 - n * u)


def _wide(*ts):
    return [t.detach().cpu().to(torch.float64) for t in ts]


def _chunks(E):
    return [slice(lo, min(lo + CHUNK_EDGES, E)) for lo in range(0, E, CHUNK_EDGES)]


def weighting(x, weight, basis, weight_index):
    """out [E, M_out] = sum_s sum_i w[wi, i, o] * b[e, s] * x[e, i]"""
    x, weight, basis = _wide(x, weight, basis)
    wi = weight_index.cpu()
    val, mag = [], []
    for c in _chunks(x.size(0)):
        terms = weight[wi[c]] * basis[c][:, :, None, None] * x[c][:, None, :, None]   # [e, S, M_in, M_out]
        val.append(terms.sum((1, 2))), mag.append(terms.abs().sum((1, 2)))
    empty = torch.zeros(0, weight.size(2), dtype=torch.float64)
    return torch.cat(val or [empty]), torch.cat(mag or [empty])


def backward_x(grad_out, weight, basis, weight_index):
    """gx [E, M_in] = sum_o sum_s g[e, o] * b[e, s] * w[wi, i, o]"""
    g, weight, basis = _wide(grad_out, weight, basis)
    wi = weight_index.cpu()
    val, mag = [], []
    for c in _chunks(g.size(0)):
        terms = weight[wi[c]] * basis[c][:, :, None, None] * g[c][:, None, None, :]
        val.append(terms.sum((1, 3))), mag.append(terms.abs().sum((1, 3)))
    empty = torch.zeros(0, weight.size(1), dtype=torch.float64)
    return torch.cat(val or [empty]), torch.cat(mag or [empty])


def backward_basis(grad_out, x, weight, weight_index):
    """gb [E, S] = sum_o sum_i g[e, o] * w[wi, i, o] * x[e, i]"""
    g, x, weight = _wide(grad_out, x, weight)
    wi = weight_index.cpu()
    val, mag = [], []
    for c in _chunks(g.size(0)):
        terms = weight[wi[c]] * x[c][:, None, :, None] * g[c][:, None, None, :]
        val.append(terms.sum((2, 3))), mag.append(terms.abs().sum((2, 3)))
    empty = torch.zeros(0, wi.size(1), dtype=torch.float64)
    return torch.cat(val or [empty]), torch.cat(mag or [empty])


def backward_weight(grad_out, x, basis, weight_index, K):
    """gw [K, M_in, M_out] = sum over the pairs with wi == k of g[e, o] * b[e, s] * x[e, i]; also the pair count per weight"""
    g, x, basis = _wide(grad_out, x, basis)
    wi = weight_index.cpu()
    E, S = wi.shape
    val = torch.zeros(K, x.size(1), g.size(1), dtype=torch.float64)
    mag = torch.zeros_like(val)
    for c in _chunks(E):
        outer = x[c][:, :, None] * g[c][:, None, :]                              # [e, M_in, M_out]
        terms = (basis[c][:, :, None, None] * outer[:, None]).flatten(0, 1)      # [e * S, M_in, M_out]
        val.index_add_(0, wi[c].flatten(), terms), mag.index_add_(0, wi[c].flatten(), terms.abs())
    return val, mag, torch.bincount(wi.flatten(), minlength=K)
