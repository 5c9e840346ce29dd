"""A plain reference of the reduce families for gradient tests: pure torch on the CPU, no project op.  Every entry takes
the arguments of the op of the same name and returns its value (min / max: the value only); hand it a float64 `src` that
requires grad and take the gradient with torch autograd -- the formulas below are dense ones (scatter_add, gather, where,
prod) whose derivatives are torch's own.

The conventions torch's scatter_reduce does not share are written out:
  min / max  the value is `src` gathered at the FIRST source position of the extremum in the order along `dim`
             (`_first_extremum`: two stable sorts), so the whole gradient goes there; an empty bucket reads 0 and passes no
             gradient.  A given `out` takes part with its own value and is beaten only by a strictly better source element.
  mul        a source element equal to 0 gets the gradient 0: the binding's `where(src != 0, grad * out / src, 0)`, taken
             from the project this one was modelled on (torch's prod would hand such an element the product of the others).
  mean       the sum divided by max(count, 1).  CSR: only positions covered by a row count, positions that no row covers
             get the gradient 0.
  softmax    exp(x - max) / sum per group, whose derivative is o * (g - sum(o * g)); positions outside every group read 0.
A given `out` is a constant here (no gradient is taken with respect to it)."""
import torch


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def _norm(dim, src):
    return dim + src.dim() if dim < 0 else dim


def broadcast_index(index, src, dim):
    """scatter_*: a 1-D index lies along `dim`; any index gets trailing dimensions and is expanded to src's shape"""
    dim = _norm(dim, src)
    if index.dim() == 1:
        index = index.reshape((1,) * dim + (-1,))
    while index.dim() < src.dim():
        index = index.unsqueeze(-1)
    return index.expand(src.shape)


def coo_index(index, src):
    """segment_*_coo / gather_coo: index is broadcast to src.shape[:index.dim()]; the reduction runs along its last dim"""
    return index.expand(src.shape[:index.dim()])


def csr_index(indptr, src, E=None):
    """The row of every position along dim = indptr.dim() - 1, shaped src.shape[:dim] + (E,); `rows` where no row covers it"""
    dim = indptr.dim() - 1
    E = src.size(dim) if E is None else E
    rows = indptr.size(-1) - 1
    ip = indptr.expand(src.shape[:dim] + (rows + 1,)).reshape(-1, rows + 1)
    idx = torch.empty((ip.size(0), E), dtype=torch.long)
    for s in range(ip.size(0)):         # plain loops: the definition, not a search
        idx[s] = rows
        for r in range(rows):
            idx[s, int(ip[s, r]):int(ip[s, r + 1])] = r
    return idx.reshape(src.shape[:dim] + (E,))


def _size(index, dim_size, out, dim):
    if out is not None:
        return out.size(dim)
    if dim_size is not None:
        return dim_size
    return int(index.max()) + 1 if index.numel() else 0


def _out_shape(src, dim, N):
    shape = list(src.shape)
    shape[dim] = N
    return shape


# ---- the four reductions over a full index -------------------------------------------------------------------------------------
def _sum(src, idx, dim, N):
    return torch.zeros(_out_shape(src, dim, N), dtype=src.dtype).scatter_add(dim, idx, src)


def _count(src, idx, dim, N):
    return _sum(torch.ones_like(src).detach(), idx, dim, N)


def _first_extremum(src, idx, dim, N, is_min):
    """arg[..., n, ...]: the first position along `dim` of the smallest (largest) element of bucket n; E for an empty one"""
    E = src.size(dim)
    lines = torch.Size(_out_shape(src, dim, 1)).numel()
    s2 = src.detach().movedim(dim, -1).reshape(lines, E)
    i2 = idx.movedim(dim, -1).reshape(lines, E)
    arg = torch.full((s2.size(0), N), E, dtype=torch.long)
    if s2.numel():
        by_value = torch.sort(s2, dim=1, descending=not is_min, stable=True).indices    # equal values stay in source order
        ids = i2.gather(1, by_value)
        by_bucket = torch.sort(ids, dim=1, stable=True).indices
        pos, ids = by_value.gather(1, by_bucket), ids.gather(1, by_bucket)
        first = torch.ones_like(ids, dtype=torch.bool)
        first[:, 1:] = ids[:, 1:] != ids[:, :-1]
        m, e = first.nonzero(as_tuple=True)
        arg[m, ids[m, e]] = pos[m, e]
    shape = list(src.movedim(dim, -1).shape)
    shape[-1] = N
    return arg.reshape(shape).movedim(-1, dim)


def _minmax(src, idx, dim, N, is_min, out=None):
    arg = _first_extremum(src, idx, dim, N, is_min)
    pad = torch.cat([src, torch.zeros(_out_shape(src, dim, 1), dtype=src.dtype)], dim)
    val = pad.gather(dim, arg)
    if out is not None:
        wins = (arg < src.size(dim)) & ((val < out) if is_min else (val > out))
        val = torch.where(wins, val, out)
        arg = torch.where(wins, arg, torch.full_like(arg, src.size(dim)))
    return val, arg


def _mul(src, idx, dim, N):
    src = torch.where(src != 0, src, src.detach())      # the convention: a zero factor passes no gradient
    buckets = torch.arange(N).reshape((N,) + (1,) * (src.dim() - dim))
    member = idx.unsqueeze(dim) == buckets              # [..., N, E, ...]
    return torch.where(member, src.unsqueeze(dim), torch.ones((), dtype=src.dtype)).prod(dim + 1)


def _reduce(op, src, idx, dim, N, out=None):
    if op == 'sum':
        res = _sum(src, idx, dim, N)
        return res if out is None else out + res
    if op == 'mul':
        res = _mul(src, idx, dim, N)
        return res if out is None else out * res
    return _minmax(src, idx, dim, N, op == 'min', out)[0]


# ---- scatter_* -----------------------------------------------------------------------------------------------------------------
def _scatter(op, src, index, dim=-1, out=None, dim_size=None):
    dim = _norm(dim, src)
    return _reduce(op, src, broadcast_index(index, src, dim), dim, _size(index, dim_size, out, dim), out)


def scatter_sum(src, index, dim=-1, out=None, dim_size=None):
    return _scatter('sum', src, index, dim, out, dim_size)


def scatter_mul(src, index, dim=-1, out=None, dim_size=None):
    return _scatter('mul', src, index, dim, out, dim_size)


def scatter_min(src, index, dim=-1, out=None, dim_size=None):
    return _scatter('min', src, index, dim, out, dim_size)


def scatter_max(src, index, dim=-1, out=None, dim_size=None):
    return _scatter('max', src, index, dim, out, dim_size)


def scatter_mean(src, index, dim=-1, out=None, dim_size=None):
    """(out + sum) / max(count, 1): a given `out` is accumulated into before the division"""
    dim = _norm(dim, src)
    idx = broadcast_index(index, src, dim)
    N = _size(index, dim_size, out, dim)
    return _reduce('sum', src, idx, dim, N, out) / _count(src, idx, dim, N).clamp(min=1)


def scatter_arg(src, index, dim, dim_size, is_min):
    """the argindex scatter_min / scatter_max return next to the value"""
    dim = _norm(dim, src)
    return _first_extremum(src, broadcast_index(index, src, dim), dim, _size(index, dim_size, None, dim), is_min)


# ---- segment_*_coo, gather_coo ---------------------------------------------------------------------------------------------------
def _coo(op, src, index, out=None, dim_size=None):
    dim = index.dim() - 1
    ib = coo_index(index, src)
    N = _size(ib, dim_size, out, dim)
    idx = broadcast_index(ib, src, dim)
    if op == 'mean':    # touched buckets are overwritten, the others keep the caller's value
        mean = _sum(src, idx, dim, N) / _count(src, idx, dim, N).clamp(min=1)
        return mean if out is None else torch.where(_count(src, idx, dim, N) > 0, mean, out)
    return _reduce(op, src, idx, dim, N, out)


def segment_sum_coo(src, index, out=None, dim_size=None):
    return _coo('sum', src, index, out, dim_size)


def segment_mean_coo(src, index, out=None, dim_size=None):
    return _coo('mean', src, index, out, dim_size)


def segment_min_coo(src, index, out=None, dim_size=None):
    return _coo('min', src, index, out, dim_size)


def segment_max_coo(src, index, out=None, dim_size=None):
    return _coo('max', src, index, out, dim_size)


def gather_coo(src, index, out=None):
    """out[..., i, ...] = src[..., index[..., i], ...]: every position of a given `out` is overwritten"""
    ib = index
    while ib.dim() < src.dim():
        ib = ib.unsqueeze(-1)
    return src.gather(index.dim() - 1, ib.expand(index.shape + src.shape[index.dim():]))


# ---- segment_*_csr, gather_csr ---------------------------------------------------------------------------------------------------
def _csr(op, src, indptr, out=None):
    dim = indptr.dim() - 1
    rows = indptr.size(-1) - 1
    idx = broadcast_index(csr_index(indptr, src), src, dim)          # uncovered positions fall into the extra bucket `rows`
    if op == 'mean':                                                  # a given `out` is overwritten
        res = _sum(src, idx, dim, rows + 1) / _count(src, idx, dim, rows + 1).clamp(min=1)
        return res.narrow(dim, 0, rows)
    pad = None
    if out is not None:
        pad = torch.cat([out, torch.zeros(_out_shape(out, dim, 1), dtype=out.dtype)], dim)
    return _reduce(op, src, idx, dim, rows + 1, pad).narrow(dim, 0, rows)


def segment_sum_csr(src, indptr, out=None):
    return _csr('sum', src, indptr, out)


def segment_mean_csr(src, indptr, out=None):
    return _csr('mean', src, indptr, out)


def segment_min_csr(src, indptr, out=None):
    return _csr('min', src, indptr, out)


def segment_max_csr(src, indptr, out=None):
    return _csr('max', src, indptr, out)


def gather_csr(src, indptr, out=None):
    """Row r goes to the positions indptr[r] .. indptr[r + 1]; the output is as long as the largest last offset, or as `out`,
    whose uncovered positions stay (those of a fresh output are unspecified: 0 here)."""
    dim = indptr.dim() - 1
    E = out.size(dim) if out is not None else (int(indptr[..., -1].max()) if src.numel() else 0)
    idx = csr_index(indptr, src, E)
    while idx.dim() < src.dim():
        idx = idx.unsqueeze(-1)
    idx = idx.expand(idx.shape[:dim + 1] + src.shape[dim + 1:])
    pad = torch.cat([src, torch.zeros(_out_shape(src, dim, 1), dtype=src.dtype)], dim)
    res = pad.gather(dim, idx)
    return res if out is None else torch.where(idx < src.size(dim), res, out)


def csr_arg(src, indptr, is_min):
    """the argindex of segment_min_csr / segment_max_csr: sentinel src.size(dim) for rows without a position"""
    dim = indptr.dim() - 1
    rows = indptr.size(-1) - 1
    idx = broadcast_index(csr_index(indptr, src), src, dim)
    return _first_extremum(src, idx, dim, rows + 1, is_min).narrow(dim, 0, rows)


# ---- softmax_csr -----------------------------------------------------------------------------------------------------------------
def softmax_csr(src, ptr, dim=0):
    dim = _norm(dim, src)
    groups = ptr.numel() - 1
    row = csr_index(ptr, src.movedim(dim, 0))      # [D]
    idx = row.reshape((1,) * dim + (-1,) + (1,) * (src.dim() - dim - 1)).expand(src.shape)
    top = _minmax(src, idx, dim, groups + 1, False)[0].detach()
    ex = (src - top.gather(dim, idx)).exp()
    res = ex / _sum(ex, idx, dim, groups + 1).gather(dim, idx)
    return torch.where(idx < groups, res, torch.zeros((), dtype=src.dtype))


def softmax_csr_backward(out, out_grad, ptr, dim=0):
    """o * (g - sum(o * g)) per group, written out (for the calls that hand the backward kernel an `out` of their own)"""
    dim = _norm(dim, out)
    groups = ptr.numel() - 1
    row = csr_index(ptr, out.movedim(dim, 0))
    idx = row.reshape((1,) * dim + (-1,) + (1,) * (out.dim() - dim - 1)).expand(out.shape)
    dot = _sum(out * out_grad, idx, dim, groups + 1).gather(dim, idx)
    return torch.where(idx < groups, out * (out_grad - dot), torch.zeros((), dtype=out.dtype))


# ---- the composites --------------------------------------------------------------------------------------------------------------
def scatter_softmax(src, index, dim=-1, dim_size=None):
    dim = _norm(dim, src)
    idx = broadcast_index(index, src, dim)
    N = _size(index, dim_size, None, dim)
    ex = (src - _minmax(src, idx, dim, N, False)[0].gather(dim, idx)).exp()
    return ex / _sum(ex, idx, dim, N).gather(dim, idx)


def scatter_log_softmax(src, index, dim=-1, dim_size=None, eps=1e-12):
    dim = _norm(dim, src)
    idx = broadcast_index(index, src, dim)
    N = _size(index, dim_size, None, dim)
    centred = src - _minmax(src, idx, dim, N, False)[0].gather(dim, idx)
    return centred - torch.log(_sum(centred.exp(), idx, dim, N).gather(dim, idx) + eps)


def scatter_std(src, index, dim=-1, out=None, dim_size=None, unbiased=True):
    """sqrt((out + sum of squared deviations) / max(count - 1, 1)); a one-element group has the value 0, where sqrt has no
    finite derivative: the gradient of its only element is NaN"""
    dim = _norm(dim, src)
    idx = broadcast_index(index, src, dim)
    N = _size(index, dim_size, out, dim)
    count = _count(src, idx, dim, N)
    dev = src - (_sum(src, idx, dim, N) / count.clamp(min=1)).gather(dim, idx)
    res = _reduce('sum', dev * dev, idx, dim, N, out)
    return (res / ((count - 1).clamp(min=1) if unbiased else count.clamp(min=1))).sqrt()


def scatter_logsumexp(src, index, dim=-1, out=None, dim_size=None, eps=1e-12):
    """max + log(sum(exp(x - max)) + eps); empty buckets read 0, or keep the value of a given `out`"""
    dim = _norm(dim, src)
    idx = broadcast_index(index, src, dim)
    N = _size(index, dim_size, out, dim)
    top, arg = _minmax(src, idx, dim, N, False)
    filled = arg < src.size(dim)
    ex = (src - top.gather(dim, idx)).exp()
    res = top + (_sum(ex, idx, dim, N) + eps).log()
    return torch.where(filled, res, torch.zeros((), dtype=src.dtype) if out is None else out)
