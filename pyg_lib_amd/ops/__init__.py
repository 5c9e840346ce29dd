"""Host-side mirror of ``pyg_lib.ops`` for the hot path (pyg_lib/ops/__init__.py).

Same names, argument meaning, defaults and error behaviour as the reference; every op runs a
hand-written gfx950 kernel through the C-ABI of include/pyg_hip.h.  Tensors must live on a HIP
device -- there is no CPU kernel and no Triton path in this package.
"""
from typing import List, Optional, Tuple

import contextlib

import torch
from torch import Tensor

from pyg_lib_amd import _capi


def segment_matmul(
    inputs: Tensor,
    ptr: Tensor,
    other: Tensor,
    bias: Optional[Tensor] = None,
) -> Tensor:
    """``out[ptr[b]:ptr[b + 1]] = inputs[ptr[b]:ptr[b + 1]] @ other[b] (+ bias[b])`` for every segment ``b`` --
    one persistent MFMA launch for all segments (interface of the reference's
    ``pyg_lib.ops.segment_matmul``, pyg_lib/ops/__init__.py:137-172).

    ``inputs`` is ``[N, K]`` on a HIP device, ``ptr`` the ``B + 1`` row boundaries (host or device; neither
    placement synchronises), ``other`` ``[B, K, M]``, ``bias`` optionally ``[B, M]``.  Returns ``[N, M]``.
    Differentiable in ``inputs``, ``other`` and ``bias``.

    HIP graphs: with ``ptr`` ON THE DEVICE the call -- forward and backward, with or without ``bias`` -- makes no host read
    and can be captured (``torch.cuda.graph``) and replayed on new ``inputs`` / ``other`` / ``bias`` AND new contents of
    ``ptr``.  A ``ptr`` on the host is staged through pinned memory that later calls reuse: such a call must NOT be captured
    (a replay would copy whatever the pinned slot holds by then; nothing refuses it yet) -- keep ``ptr`` on the device.
    """
    needs_grad = torch.is_grad_enabled() and (inputs.requires_grad or other.requires_grad or
                                              (bias is not None and bias.requires_grad))
    if bias is not None and not needs_grad:
        # bias as a fused GEMM epilogue (the reference: B python-side slice adds, :169-171)
        return torch.ops.pyg.segment_matmul_bias(inputs, ptr, other, bias)
    out = torch.ops.pyg.segment_matmul(inputs, ptr, other)
    if bias is not None and ptr.is_cuda:
        # row r of the bias to the rows ptr[r] .. ptr[r + 1] on the device (slicing by a device `ptr` would read every
        # boundary back: B synchronisations, and nothing a graph could hold); the same single rounding per element, and
        # rows behind ptr[B] get no bias
        rows = gather_csr(bias.to(out.dtype), ptr, out=torch.zeros_like(out))
        out = out + rows
    elif bias is not None:
        for i in range(ptr.numel() - 1):
            out[ptr[i]:ptr[i + 1]] += bias[i]
    return out


# ---------------------------------------------------------------------------------------------------
# grouped_matmul
# ---------------------------------------------------------------------------------------------------

def _grouped_matmul_fwd(inputs: List[Tensor], others: List[Tensor]) -> List[Tensor]:
    return list(torch.ops.pyg.grouped_matmul(list(inputs), list(others)))


class _GroupedMatmul(torch.autograd.Function):
    """Mirrors GroupedMatmul (pyg_lib/ops/__init__.py:59-96) without the pytree indirection:
    the flat argument tuple is `inputs + others`."""
    @staticmethod
    def forward(ctx, *args: Tensor):
        ctx.save_for_backward(*args)
        n = len(args) // 2
        outs = _grouped_matmul_fwd(list(args[:n]), list(args[n:]))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *outs_grad: Tensor):
        args = ctx.saved_tensors
        n = len(outs_grad)
        inputs, others = list(args[:n]), list(args[n:])
        inputs_grad = [None] * n
        if any(x.requires_grad for x in inputs):
            inputs_grad = _grouped_matmul_fwd([g.contiguous() for g in outs_grad], [o.t() for o in others])
        others_grad = [None] * n
        if any(o.requires_grad for o in others):
            others_grad = _grouped_matmul_fwd([x.t() for x in inputs], [g.contiguous() for g in outs_grad])
        return tuple(inputs_grad + others_grad)


def grouped_matmul(
    inputs: List[Tensor],
    others: List[Tensor],
    biases: Optional[List[Tensor]] = None,
) -> List[Tensor]:
    """``outs[i] = inputs[i] @ others[i] (+ biases[i])`` for lists of independent 2-D operands
    (``[N_i, K_i]`` x ``[K_i, M_i]``) in one launch (interface of the reference's
    ``pyg_lib.ops.grouped_matmul``, pyg_lib/ops/__init__.py:99-134).  Differentiable.

    The group descriptors are planned on the host and staged through pinned memory that later calls reuse.  The call does
    not synchronise, but it must NOT be captured into a HIP graph: a replay would copy whatever the pinned slot holds by
    then (nothing refuses it yet).  Call it outside the capture, or use :func:`segment_matmul` with ``ptr`` on the device.
    """
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in list(inputs) + list(others))
    if needs_grad:
        outs = list(_GroupedMatmul.apply(*(list(inputs) + list(others))))
    else:
        outs = _grouped_matmul_fwd(list(inputs), list(others))
    if biases is not None:
        for i in range(len(biases)):
            outs[i] = outs[i] + biases[i]
    return outs


# ---------------------------------------------------------------------------------------------------
# sampled_add / sub / mul / div  (pyg_lib/ops/__init__.py:175-292)
# ---------------------------------------------------------------------------------------------------

def sampled_add(
    left: Tensor,
    right: Tensor,
    left_index: Optional[Tensor] = None,
    right_index: Optional[Tensor] = None,
) -> Tensor:
    r"""Edge-level sum of two node tensors: ``out[e] = left[left_index[e]] + right[right_index[e]]``, computed in
    one pass so that neither gathered operand is written to memory (three row passes instead of seven).

    :obj:`left` and :obj:`right` are contiguous ``[N_left, F]`` / ``[N_right, F]`` tensors of one dtype and device.
    An index is a contiguous 1-D int64 or int32 tensor of ``E`` row numbers; :obj:`None` reads its tensor row by row
    (which then must have ``E`` rows).  Returns ``[E, F]``.  Differentiable in :obj:`left` and :obj:`right`: the
    gradient of an indexed side is summed per row through :func:`scatter_sum`, so it is reproducible on large
    inputs and follows ``torch.use_deterministic_algorithms``.  On a HIP device the indices are not range-checked.
    """
    return torch.ops.pyg.sampled_op(left, right, left_index, right_index, 'add')


def sampled_sub(
    left: Tensor,
    right: Tensor,
    left_index: Optional[Tensor] = None,
    right_index: Optional[Tensor] = None,
) -> Tensor:
    r"""Edge-level difference ``out[e] = left[left_index[e]] - right[right_index[e]]`` in one pass; arguments,
    result and gradients as for :func:`sampled_add`."""
    return torch.ops.pyg.sampled_op(left, right, left_index, right_index, 'sub')


def sampled_mul(
    left: Tensor,
    right: Tensor,
    left_index: Optional[Tensor] = None,
    right_index: Optional[Tensor] = None,
) -> Tensor:
    r"""Edge-level product ``out[e] = left[left_index[e]] * right[right_index[e]]`` in one pass; arguments, result
    and gradients as for :func:`sampled_add`."""
    return torch.ops.pyg.sampled_op(left, right, left_index, right_index, 'mul')


def sampled_div(
    left: Tensor,
    right: Tensor,
    left_index: Optional[Tensor] = None,
    right_index: Optional[Tensor] = None,
) -> Tensor:
    r"""Edge-level quotient ``out[e] = left[left_index[e]] / right[right_index[e]]`` in one pass (true division,
    correctly rounded); arguments, result and gradients as for :func:`sampled_add`.  Floating-point tensors only on
    a HIP device: integer division raises there."""
    return torch.ops.pyg.sampled_op(left, right, left_index, right_index, 'div')


# ---------------------------------------------------------------------------------------------------
# fused_scatter_reduce  (pyg_lib/ops/scatter_reduce.py:95-181)
# ---------------------------------------------------------------------------------------------------

def fused_scatter_reduce(inputs: Tensor, index: Tensor, dim_size: int, reduce_list: List[str]) -> Tensor:
    r"""Several reductions of :obj:`inputs` over one :obj:`index` in one sort and one pass over the rows (multi-aggregation,
    ``aggr=['sum', 'mean', 'min', 'max']``): ``out[:, i * F:(i + 1) * F]`` holds ``reduce_list[i]``.

    :obj:`inputs` is a contiguous floating-point ``[E, F]`` tensor (float32, float64, bfloat16 or float16), :obj:`index` a
    contiguous int64 ``[E]`` tensor of bucket numbers in ``[0, dim_size)`` on the same device; :obj:`reduce_list` holds one
    to four distinct names out of ``'sum'``, ``'mean'``, ``'min'``, ``'max'`` in any order.  Returns
    ``[dim_size, len(reduce_list) * F]``.

    A bucket is reduced in source order with float32 accumulators (float64 for float64) and rounded once; ``mean`` is that
    sum divided by ``max(count, 1)``.  Empty buckets give 0 in every slice; a NaN never wins ``min`` / ``max`` and makes
    ``sum`` / ``mean`` NaN; ``+0`` and ``-0`` tie and the first one stays.  No float atomics: the result is the same on every
    run and unchanged under ``torch.use_deterministic_algorithms(True)``.  Differentiable in :obj:`inputs`: the gradient of
    ``min`` / ``max`` goes to the first position that produced the value, as for :func:`scatter_min`.  The positions are
    computed only when :obj:`inputs` requires grad.  On a HIP device :obj:`index` is not range-checked, the call never
    synchronises and can be captured in a graph.
    """
    return torch.ops.pyg.fused_scatter_reduce(inputs, index, dim_size, list(reduce_list))


# ---------------------------------------------------------------------------------------------------
# index_sort
# ---------------------------------------------------------------------------------------------------

def index_sort(
    inputs: Tensor,
    max_value: Optional[int] = None,
) -> Tuple[Tensor, Tensor]:
    """Stable ascending sort of a 1-D tensor of non-negative integers; returns ``(sorted values,
    permutation)`` and equals ``torch.sort(inputs, stable=True)`` (interface of the reference's
    ``pyg_lib.ops.index_sort``, pyg_lib/ops/__init__.py:295-321).  ``max_value`` -- any upper bound of the
    keys -- limits the number of radix passes.  The reference hands device tensors to ``torch.sort``
    (:319-320); here they run this library's LDS radix sort.
    """
    return torch.ops.pyg.index_sort(inputs, max_value)


# ---------------------------------------------------------------------------------------------------
# scatter / segment_coo / gather_coo  (pyg_lib/ops/__init__.py:353-631, 764-835)
# ---------------------------------------------------------------------------------------------------

def scatter_sum(src: Tensor, index: Tensor, dim: int = -1, out: Optional[Tensor] = None,
                dim_size: Optional[int] = None) -> Tensor:
    r"""Reduces all values from :obj:`src` into :obj:`out` at the indices specified in :obj:`index`
    along :obj:`dim`, using ``sum``.  A fresh :obj:`out` is zero-initialised; a given :obj:`out` is
    **accumulated** into (pyg_lib/ops/__init__.py:353-380)."""
    return torch.ops.pyg.scatter_sum(src, index, dim, out, dim_size)


scatter_add = scatter_sum


def scatter_mul(src: Tensor, index: Tensor, dim: int = -1, out: Optional[Tensor] = None,
                dim_size: Optional[int] = None) -> Tensor:
    r"""``mul`` reduction; a fresh :obj:`out` starts from ones, a given one is multiplied into."""
    return torch.ops.pyg.scatter_mul(src, index, dim, out, dim_size)


def scatter_mean(src: Tensor, index: Tensor, dim: int = -1, out: Optional[Tensor] = None,
                 dim_size: Optional[int] = None) -> Tensor:
    r"""``mean`` reduction (sum / count, floor division for integer dtypes; empty buckets give 0)."""
    return torch.ops.pyg.scatter_mean(src, index, dim, out, dim_size)


def scatter_min(src: Tensor, index: Tensor, dim: int = -1, out: Optional[Tensor] = None,
                dim_size: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    r"""``min`` reduction.  Returns ``(values, argindex)``; empty buckets yield value ``0`` and
    argindex ``src.size(dim)`` (sentinel); on ties the first source position wins."""
    return torch.ops.pyg.scatter_min(src, index, dim, out, dim_size)


def scatter_max(src: Tensor, index: Tensor, dim: int = -1, out: Optional[Tensor] = None,
                dim_size: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    r"""``max`` reduction.  Returns ``(values, argindex)`` (see :func:`scatter_min`)."""
    return torch.ops.pyg.scatter_max(src, index, dim, out, dim_size)


def segment_sum_coo(src: Tensor, index: Tensor, out: Optional[Tensor] = None,
                    dim_size: Optional[int] = None) -> Tensor:
    r"""Sums :obj:`src` over the runs of a **sorted** :obj:`index` along ``index.dim() - 1``."""
    return torch.ops.pyg.segment_sum_coo(src, index, out, dim_size)


segment_add_coo = segment_sum_coo


def segment_mean_coo(src: Tensor, index: Tensor, out: Optional[Tensor] = None,
                     dim_size: Optional[int] = None) -> Tensor:
    r"""Mean over the runs of a sorted :obj:`index`; buckets touched by :obj:`index` are overwritten."""
    return torch.ops.pyg.segment_mean_coo(src, index, out, dim_size)


def segment_min_coo(src: Tensor, index: Tensor, out: Optional[Tensor] = None,
                    dim_size: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    r"""Min over the runs of a sorted :obj:`index`; returns ``(values, argindex)``."""
    return torch.ops.pyg.segment_min_coo(src, index, out, dim_size)


def segment_max_coo(src: Tensor, index: Tensor, out: Optional[Tensor] = None,
                    dim_size: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    r"""Max over the runs of a sorted :obj:`index`; returns ``(values, argindex)``."""
    return torch.ops.pyg.segment_max_coo(src, index, out, dim_size)


def gather_coo(src: Tensor, index: Tensor, out: Optional[Tensor] = None) -> Tensor:
    r"""``out[..., i, ...] = src[..., index[..., i], ...]`` along ``index.dim() - 1``."""
    return torch.ops.pyg.gather_coo(src, index, out)


def scatter(src: Tensor, index: Tensor, dim: int = -1, out: Optional[Tensor] = None,
            dim_size: Optional[int] = None, reduce: str = 'sum') -> Tensor:
    r"""Routes to the typed scatter op by :obj:`reduce` (``"sum"``/``"add"``, ``"mul"``, ``"mean"``,
    ``"min"``, ``"max"``); min/max return only the values (pyg_lib/ops/__init__.py:764-791)."""
    if reduce == 'sum' or reduce == 'add':
        return scatter_sum(src, index, dim, out, dim_size)
    if reduce == 'mul':
        return scatter_mul(src, index, dim, out, dim_size)
    if reduce == 'mean':
        return scatter_mean(src, index, dim, out, dim_size)
    if reduce == 'min':
        return scatter_min(src, index, dim, out, dim_size)[0]
    if reduce == 'max':
        return scatter_max(src, index, dim, out, dim_size)[0]
    raise ValueError(f'Unknown reduce: {reduce!r}')


def segment_coo(src: Tensor, index: Tensor, out: Optional[Tensor] = None, dim_size: Optional[int] = None,
                reduce: str = 'sum') -> Tensor:
    r"""Routes by :obj:`reduce` to the typed ``segment_*_coo`` op (pyg_lib/ops/__init__.py:794-813)."""
    if reduce == 'sum' or reduce == 'add':
        return segment_sum_coo(src, index, out, dim_size)
    if reduce == 'mean':
        return segment_mean_coo(src, index, out, dim_size)
    if reduce == 'min':
        return segment_min_coo(src, index, out, dim_size)[0]
    if reduce == 'max':
        return segment_max_coo(src, index, out, dim_size)[0]
    raise ValueError(f'Unknown reduce: {reduce!r}')


def _broadcast(index: Tensor, src: Tensor, dim: int) -> Tensor:
    if dim < 0:
        dim = src.dim() + dim
    if index.dim() == 1:
        for _ in range(dim):
            index = index.unsqueeze(0)
    for _ in range(index.dim(), src.dim()):
        index = index.unsqueeze(-1)
    return index.expand(src.size())


def _require_float(name: str, src: Tensor) -> None:
    if not src.is_floating_point():
        raise ValueError(f'{name} requires a floating-point src tensor (got {src.dtype})')


def _require_no_grad_out(name: str, out: Optional[Tensor]) -> None:
    # as the typed ops: no gradient is computed for a given `out`
    if out is not None and out.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"{name}: the gradient with respect to a given 'out' is not implemented ('out' requires grad); "
                           f"pass out.detach() or call under torch.no_grad()")


def scatter_softmax(src: Tensor, index: Tensor, dim: int = -1, dim_size: Optional[int] = None) -> Tensor:
    r"""Softmax over the groups given by :obj:`index` (pyg_lib/ops/__init__.py:838-862): recentre by
    the per-group max, exponentiate, divide by the per-group sum."""
    _require_float('scatter_softmax', src)
    idx = _broadcast(index, src, dim)
    group_max = scatter_max(src, index, dim, dim_size=dim_size)[0]
    ex = (src - group_max.gather(dim, idx)).exp()
    group_sum = scatter_sum(ex, index, dim, dim_size=dim_size)
    return ex / group_sum.gather(dim, idx)


def scatter_log_softmax(src: Tensor, index: Tensor, dim: int = -1, dim_size: Optional[int] = None,
                        eps: float = 1e-12) -> Tensor:
    r"""Log-softmax over the groups given by :obj:`index` (pyg_lib/ops/__init__.py:865-889)."""
    _require_float('scatter_log_softmax', src)
    idx = _broadcast(index, src, dim)
    group_max = scatter_max(src, index, dim, dim_size=dim_size)[0]
    centred = src - group_max.gather(dim, idx)
    group_sum = scatter_sum(centred.exp(), index, dim, dim_size=dim_size)
    return centred - torch.log(group_sum.gather(dim, idx) + eps)


def scatter_std(src: Tensor, index: Tensor, dim: int = -1, out: Optional[Tensor] = None,
                dim_size: Optional[int] = None, unbiased: bool = True) -> Tensor:
    r"""Standard deviation per group (pyg_lib/ops/__init__.py:892-931): two :func:`scatter_sum`
    passes, Bessel's correction ``N / (N - 1)`` when :obj:`unbiased`.  A group of one element has the value 0, where the
    square root has no finite derivative: the gradient is NaN for that one element and right for every other, as in the
    reference."""
    _require_float('scatter_std', src)
    _require_no_grad_out('scatter_std', out)
    if out is not None:
        dim_size = out.size(dim)
    idx = _broadcast(index, src, dim)
    count = scatter_sum(torch.ones_like(src), idx, dim, dim_size=dim_size)
    total = scatter_sum(src, idx, dim, dim_size=dim_size)
    count_safe = count.clamp(min=1)
    dev = src - (total / count_safe).gather(dim, idx)
    res = scatter_sum(dev * dev, idx, dim, out, dim_size)
    denom = (count - 1).clamp(min=1) if unbiased else count_safe
    return (res / denom).sqrt()


def scatter_logsumexp(src: Tensor, index: Tensor, dim: int = -1, out: Optional[Tensor] = None,
                      dim_size: Optional[int] = None, eps: float = 1e-12) -> Tensor:
    r"""Numerically stable log-sum-exp per group (pyg_lib/ops/__init__.py:934-984).  Empty buckets
    give ``0`` for a fresh output and keep the caller's value when :obj:`out` is supplied."""
    _require_float('scatter_logsumexp', src)
    _require_no_grad_out('scatter_logsumexp', out)
    if out is not None:
        dim_size = out.size(dim)
    size = list(src.size())
    if dim_size is not None:
        size[dim] = dim_size
    elif index.numel() == 0:
        size[dim] = 0
    else:
        size[dim] = int(index.max().item()) + 1
    group_max = torch.full(size, float('-inf'), dtype=src.dtype, device=src.device)
    scatter_max(src, index, dim, group_max, dim_size)
    idx = _broadcast(index, src, dim)
    centred = src - group_max.gather(dim, idx)
    centred = torch.where(torch.isnan(centred), torch.full_like(centred, float('-inf')), centred)
    group_sum = scatter_sum(centred.exp(), index, dim, dim_size=dim_size)
    res = group_max + (group_sum + eps).log()
    if out is None:
        return res.nan_to_num(nan=0.0, posinf=0.0, neginf=0.0)
    keep = out.clone()
    out.copy_(torch.where(~torch.isfinite(res), keep, res))
    return out


# ---- CSR family (pyg_lib/ops/__init__.py:324-350, 634-745, 816-836) -----------------------------------
def softmax_csr(src: Tensor, ptr: Tensor, dim: int = 0) -> Tensor:
    r"""Sparsely evaluated softmax: groups the values of :obj:`src` along :obj:`dim` by the CSR
    pointer :obj:`ptr` and normalises every group on its own (pyg_lib/ops/__init__.py:324-350)."""
    dim = dim + src.dim() if dim < 0 else dim
    return torch.ops.pyg.softmax_csr(src, ptr, dim)


def segment_sum_csr(src: Tensor, indptr: Tensor, out: Optional[Tensor] = None) -> Tensor:
    r"""Row sums of :obj:`src` along ``indptr.dim() - 1`` by the CSR pointer :obj:`indptr`
    (``[..., R+1]``); a given :obj:`out` is **accumulated** into."""
    return torch.ops.pyg.segment_sum_csr(src, indptr, out)


segment_add_csr = segment_sum_csr


def segment_mean_csr(src: Tensor, indptr: Tensor, out: Optional[Tensor] = None) -> Tensor:
    r"""Row means (empty rows read 0); a given :obj:`out` is overwritten."""
    return torch.ops.pyg.segment_mean_csr(src, indptr, out)


def segment_min_csr(src: Tensor, indptr: Tensor, out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    r"""Row minima and the source position of the first one (sentinel ``src.size(dim)`` for rows
    without a contribution)."""
    return torch.ops.pyg.segment_min_csr(src, indptr, out)


def segment_max_csr(src: Tensor, indptr: Tensor, out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    r"""Row maxima and the source position of the first one."""
    return torch.ops.pyg.segment_max_csr(src, indptr, out)


def gather_csr(src: Tensor, indptr: Tensor, out: Optional[Tensor] = None) -> Tensor:
    r"""Inverse of :func:`segment_sum_csr`: row ``r`` of :obj:`src` is written to the positions
    ``indptr[r] .. indptr[r+1]`` of the output."""
    return torch.ops.pyg.gather_csr(src, indptr, out)


def segment_csr(src: Tensor, indptr: Tensor, out: Optional[Tensor] = None, reduce: str = 'sum') -> Tensor:
    r"""Polymorphic CSR segment dispatcher; min/max return only the value tensor."""
    if reduce == 'sum' or reduce == 'add':
        return segment_sum_csr(src, indptr, out)
    if reduce == 'mean':
        return segment_mean_csr(src, indptr, out)
    if reduce == 'min':
        return segment_min_csr(src, indptr, out)[0]
    if reduce == 'max':
        return segment_max_csr(src, indptr, out)[0]
    raise ValueError(f'Unknown reduce: {reduce!r}')


def matmul_last_variant() -> str:
    """Name of the kernel variant the last matmul call dispatched to (test/diagnostic hook)."""
    return _capi.lib().pyg_hip_matmul_last_variant().decode()


def scatter_last_route() -> str:
    """Name of the route the last ``pyg_hip_scatter`` call made FROM THE CALLING THREAD took -- the last ``scatter_*`` /
    ``segment_*_coo`` op, for ``scatter_mean`` its count (test/diagnostic hook): ``'csr_rows'`` / ``'sort_rows'`` (atomic-free
    CSR rows: sorted index / after an index sort), ``'vec_sorted'`` / ``'vec_unsorted'`` / ``'pair'`` / ``'elem'`` (atomic sums;
    ``'elem'`` also mul), ``'atomic'`` (min / max), ``'none'`` (nothing to do); the rules are the table of ``pyg_hip_scatter``
    in include/pyg_hip.h."""
    return _capi.lib().pyg_hip_scatter_last_route().decode()


def csr_last_route() -> str:
    """What the last CSR launch made FROM THE CALLING THREAD was made of (test/diagnostic hook): the last ``segment_*_csr`` /
    ``gather_csr`` / ``softmax_csr`` op, or the rows back end of a ``scatter_*`` / ``segment_*_coo`` op that took the
    ``'csr_rows'`` / ``'sort_rows'`` route -- ``'<segment|gather|softmax|softmax_bwd> <kernel> v<V> <hub mode>[ ch<CH>]'``,
    ``'none'`` or ``'unsupported'``; the rules are the table of ``pyg_hip_csr_route`` in include/pyg_hip.h."""
    return _capi.lib().pyg_hip_csr_last_route().decode()


def matmul_dw_counters() -> Tuple[int, int]:
    """(specialised, general): calls served by the shape-specialised / the general-shape weight-gradient kernels since the
    library was loaded (process wide -- the backward pass runs on an autograd thread)."""
    import ctypes
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    _capi.lib().pyg_hip_matmul_dw_counters(ctypes.byref(a), ctypes.byref(b))
    return int(a.value), int(b.value)


_SCHEDULES = {'auto': 0, 'contiguous': 1, 'cyclic': 2, 'ticket': 3, 'general': 4, 'naive': 5, 'ring': 6}


def set_matmul_schedule(mode: str = 'auto') -> None:
    """Tile schedule / kernel family of the matmul calls made FROM THE CALLING THREAD (a test and measurement hook; the
    backward of a ``segment_matmul`` inherits the schedule its forward ran with).  It becomes the ``PYG_HIP_MM_SCHED_*``
    bits of the ``flags`` argument of ``pyg_hip_segment_matmul`` / ``pyg_hip_grouped_matmul`` (include/pyg_hip.h):

    * ``'auto'`` (default): ticket schedule for long relations, item ring for many short ones, contiguous ranges for
      small calls;
    * 16-bit ``K = M = 128``: ``'contiguous'`` (one tile range per workgroup), ``'cyclic'`` (every XCD sweeps its band of
      tiles), ``'ticket'`` (tiles drawn in address order from per-XCD counters, W in registers), ``'ring'`` (W slices in
      registers, X tiles through an LDS-DMA item ring) -- the same bits from each, they differ in speed only;
    * 16-bit ``K = M = 256``: ``'auto'`` / ``'ring'`` = W in registers + item ring, ``'contiguous'`` = W in LDS with 32
      rows per wave, ``'cyclic'`` / ``'ticket'`` = W in LDS with 64 rows per wave;
    * fp32 ``K = M = 128`` in split-bf16 arithmetic: ``'ring'`` forces the register-W ring kernel;
    * ``'general'`` / ``'naive'`` (measurement only): every floating-point shape through the general-shape MFMA kernel /
      every call through the one-thread-per-output kernel.

    fp32 arithmetic is not selected here: it follows ``torch.get_float32_matmul_precision()`` as in the reference
    (``'highest'``, torch's default: IEEE fp32 MFMAs; ``'high'`` / ``'medium'``: the split-bf16 kernels for
    ``K = 128, M % 128 == 0``)."""
    _capi.binding().pyg_binding_set_matmul_schedule(_SCHEDULES[mode])


@contextlib.contextmanager
def matmul_f32_split(on: bool = True):
    """Context manager over ``torch.set_float32_matmul_precision``: ``True`` -> ``'high'`` (fp32 ``K = 128, M % 128 == 0``
    matmuls run the split-bf16 kernels: three bf16 planes per operand, fp32 accumulation, HBM-bound), ``False`` ->
    ``'highest'`` (IEEE fp32 MFMAs; torch's default).  Restores the previous setting on exit.  Note that the switch is
    torch's own process-wide one -- the same the reference consults (ops/cuda/matmul_kernel.cu:158-165)."""
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('high' if on else 'highest')
    try:
        yield
    finally:
        torch.set_float32_matmul_precision(prev)


# ---------------------------------------------------------------------------------------------------
# knn, radius, nearest (csrc/hip/spatial.hip)
# ---------------------------------------------------------------------------------------------------

def knn(
    x: Tensor,
    y: Tensor,
    k: int = 1,
    ptr_x: Optional[Tensor] = None,
    ptr_y: Optional[Tensor] = None,
    cosine: bool = False,
    num_workers: int = 1,
) -> Tensor:
    """For every point of ``y`` ``[M, D]`` the ``k`` nearest points of ``x`` ``[N, D]`` inside its example (interface of the
    reference's ``pyg_lib.ops.knn``; note that ``k`` comes before the pointers here and after them in the operator schema).

    ``ptr_x`` / ``ptr_y`` are int64 CSR pointers of equal length on the points' device; without them there is one example.
    Returns ``[2, E]`` int64: row 0 the index into ``y``, row 1 the index into ``x``; per query the neighbours are ordered by
    (squared Euclidean distance, index) and there are ``min(k, candidates)`` of them -- candidates at a NaN or infinite
    distance do not count.  The distance is summed in fp32 (fp64 for float64 inputs) without fused multiply-add, so HIP and CPU
    tensors give the same bits.  ``cosine=True`` (device only) uses ``1 - cos``.  On the device ``k <= 100``.  ``num_workers``
    is accepted and ignored.  Reads the pair count back: one synchronisation of the current stream per call."""
    return torch.ops.pyg.knn(x, y, ptr_x, ptr_y, k, cosine, num_workers)


def radius(
    x: Tensor,
    y: Tensor,
    r: float = 1.0,
    ptr_x: Optional[Tensor] = None,
    ptr_y: Optional[Tensor] = None,
    max_num_neighbors: int = 32,
    num_workers: int = 1,
    ignore_same_index: bool = False,
) -> Tensor:
    """For every point of ``y`` ``[M, D]`` the points of ``x`` ``[N, D]`` of its example at a distance below ``r`` (strictly:
    ``dist < r * r``), at most the first ``max_num_neighbors`` in ascending index (interface of the reference's
    ``pyg_lib.ops.radius``).  Returns ``[2, E]`` int64 ordered by (index into ``y``, index into ``x``) on both devices -- the
    rule of the reference's CUDA kernel; its CPU kernel returns KD-tree order.  ``ignore_same_index`` drops
    the pairs ``(i, i)``.  One synchronisation of the current stream per call."""
    return torch.ops.pyg.radius(x, y, ptr_x, ptr_y, r, max_num_neighbors, num_workers, ignore_same_index)


def nearest(
    x: Tensor,
    y: Tensor,
    ptr_x: Optional[Tensor] = None,
    ptr_y: Optional[Tensor] = None,
) -> Tensor:
    """For every point of ``x`` ``[N, D]`` the index of the nearest point of ``y`` ``[M, D]`` inside its example: the first one
    at the smallest distance (interface of the reference's ``pyg_lib.ops.nearest``).  A point whose example has no candidate
    at a finite distance gets ``ptr_y[b]`` -- as in the reference; this can equal ``y.size(0)``.  Does not synchronise (and can
    be captured into a graph): a pointer that decreases or does not end at the row count is clamped, and reported by the NEXT
    ``nearest`` call on that device."""
    return torch.ops.pyg.nearest(x, y, ptr_x, ptr_y)


def spatial_last_route() -> str:
    """What the last ``knn`` / ``radius`` / ``nearest`` call made from the calling thread on a HIP device ran:
    ``'<op> <lane|split> <d4|ldsq|globq> <reg1|reg16|lds|count>[ cosine]'`` (test / diagnostic hook; the rules are in
    include/pyg_hip.h)."""
    return _capi.lib().pyg_hip_spatial_last_route().decode()


@contextlib.contextmanager
def spatial_route(route: Optional[str]):
    """Context manager: the ``knn`` / ``radius`` / ``nearest`` calls of this thread take the ``'lane'`` or the ``'split'``
    route whatever their sizes (``None``: the library's rule).  For tests and measurements; a forced split uses chunks of
    at least 32 candidates, so that small inputs span several."""
    flags = {None: 0, 'lane': 1, 'split': 2}[route]   # PYG_HIP_SPATIAL_FORCE_*
    prev = _capi.binding().pyg_binding_get_spatial_route()
    _capi.binding().pyg_binding_set_spatial_route(flags)
    try:
        yield
    finally:
        _capi.binding().pyg_binding_set_spatial_route(prev)


# ---------------------------------------------------------------------------------------------------
# fps, grid_cluster (csrc/hip/downsample.hip)
# ---------------------------------------------------------------------------------------------------

def fps(src: Tensor, ptr: Tensor, ratio: float = 0.5, random_start: bool = True) -> Tensor:
    """Farthest point sampling inside every example (interface of the reference's ``pyg_lib.ops.fps``).

    ``src`` is ``[N, ...]`` (viewed as ``[N, D]``; float32, float64, float16 or bfloat16), ``ptr`` an int64 CSR pointer of
    ``B + 1`` entries on the same device, ``ratio`` in ``(0, 1]``.  Example ``b`` contributes ``ceil(float32(n_b) * ratio)``
    global point indices: its first sample is point 0 of the example, or a point drawn from the device's default generator
    (``random_start``); every further sample is the point farthest (squared Euclidean distance, summed in fp32 -- fp64 for
    float64 -- without fused multiply-add) from the samples so far, the lowest index among equals.  HIP and CPU tensors give
    the same bits.  An example without points contributes nothing.  One small device-to-host copy per call (the sizes); a
    ``ptr`` that is not non-decreasing from 0 to ``N`` raises."""
    return torch.ops.pyg.fps(src, ptr, ratio, random_start)


def grid_cluster(pos: Tensor, size: Tensor, start: Optional[Tensor] = None, end: Optional[Tensor] = None) -> Tensor:
    """The voxel id of every point of ``pos`` ``[N, ...]`` (viewed as ``[N, D]``) on a regular grid of cell ``size`` ``[D]``
    between ``start`` and ``end`` ``[D]`` (default: the column minima / maxima of ``pos``), as int64 ``[N]`` (interface of the
    reference's ``pyg_lib.ops.grid_cluster``).  ``size``, ``start`` and ``end`` have ``pos``'s dtype and device.  Never
    synchronises: it can be captured into a graph."""
    return torch.ops.pyg.grid_cluster(pos, size, start, end)


def fps_last_route() -> str:
    """What the last ``fps`` call made from the calling thread on a HIP device ran: ``'resident <d4|lds|glob> t<threads>'``,
    ``'stream <d4|glob>'`` or ``'multi <d4|glob> g<blocks>'`` (test / diagnostic hook; the rules are in include/pyg_hip.h)."""
    return _capi.lib().pyg_hip_fps_last_route().decode()


@contextlib.contextmanager
def fps_route(route: Optional[str]):
    """Context manager: the ``fps`` calls of this thread take the ``'resident'``, ``'stream'`` or ``'multi'`` route whatever
    their sizes (``None``: the library's rule).  For tests and measurements; a forced ``'resident'`` call whose largest
    example exceeds the resident capacity takes ``'stream'``, a forced ``'multi'`` call cuts slices of at least 64 points."""
    flags = {None: 0, 'resident': 1, 'stream': 2, 'multi': 3}[route]   # PYG_HIP_FPS_FORCE_*
    prev = _capi.binding().pyg_binding_get_fps_route()
    _capi.binding().pyg_binding_set_fps_route(flags)
    try:
        yield
    finally:
        _capi.binding().pyg_binding_set_fps_route(prev)


# ---------------------------------------------------------------------------------------------------
# spline_basis, spline_weighting (csrc/hip/spline.hip)
# ---------------------------------------------------------------------------------------------------

def spline_basis(pseudo: Tensor, kernel_size: Tensor, is_open_spline: Tensor, degree: int = 1) -> Tuple[Tensor, Tensor]:
    """The B-spline basis of ``SplineConv`` (interface of the reference's ``pyg_lib.ops.spline_basis``).

    ``pseudo`` is ``[E, D]`` pseudo-coordinates in ``[0, 1]``, ``kernel_size`` an int64 ``[D]`` and ``is_open_spline`` a uint8
    ``[D]`` tensor on its device, ``degree`` 1, 2 or 3.  Returns ``basis`` ``[E, (degree + 1)^D]`` in ``pseudo``'s dtype
    (differentiable in ``pseudo``) and the int64 ``weight_index`` of the same shape.  float32 and float64 on a HIP device
    (bfloat16 too on the CPU); both devices give the same bits.  Never synchronises."""
    return torch.ops.pyg.spline_basis(pseudo, kernel_size, is_open_spline, degree)


def spline_weighting(x: Tensor, weight: Tensor, basis: Tensor, weight_index: Tensor) -> Tensor:
    """``out[e] = sum_s basis[e, s] * (x[e] @ weight[weight_index[e, s]])`` (interface of the reference's
    ``pyg_lib.ops.spline_weighting``): ``x`` ``[E, M_in]``, ``weight`` ``[K, M_in, M_out]``, ``basis`` / ``weight_index``
    ``[E, S]``; differentiable in ``x``, ``weight`` and ``basis``.  float32, float64 and bfloat16.  No atomics anywhere: float32
    and float64 results have the bits of the CPU key (the weight gradient: for weights of up to 1024 pairs; bounded and
    reproducible beyond).  Never synchronises: on a HIP device a ``weight_index`` outside ``[0, K)`` contributes nothing and is
    reported by the NEXT spline call on that device (:func:`spline_pending_error`); on the CPU it raises."""
    return torch.ops.pyg.spline_weighting(x, weight, basis, weight_index)


def spline_last_route() -> str:
    """What the last ``spline_weighting`` forward, ``backward_x`` or ``backward_basis`` made from the calling thread on a HIP
    device ran: ``'<forward|backward_x|backward_basis> <lds|global> tx<lanes> te<edges>'`` (test / diagnostic hook; the rule is
    in include/pyg_hip.h)."""
    return _capi.lib().pyg_hip_spline_last_route().decode()


@contextlib.contextmanager
def spline_route(route: Optional[str]):
    """Context manager: the ``spline_weighting`` operators called from this thread take the ``'lds'`` or the ``'global'`` route
    (``None``: the library's rule, which is ``'global'`` for every shape -- ``'lds'`` measured slower and runs only when
    forced).  For tests and measurements; a forced ``'lds'`` call whose weights do not fit the LDS budget runs ``'global'``.
    Autograd's backward runs on its own thread and keeps the rule."""
    flags = {None: 0, 'lds': 1, 'global': 2}[route]   # PYG_HIP_SPLINE_FORCE_*
    prev = _capi.binding().pyg_binding_get_spline_route()
    _capi.binding().pyg_binding_set_spline_route(flags)
    try:
        yield
    finally:
        _capi.binding().pyg_binding_set_spline_route(prev)


def spline_pending_error() -> int:
    """Returns and clears the word a spline call on the current HIP device sets when it meets a ``weight_index`` outside
    ``[0, K)`` (non-zero: there was one).  Meaningful once the stream has been synchronised."""
    return int(_capi.lib().pyg_hip_spline_pending_error())


# ---------------------------------------------------------------------------------------------------
# graclus_cluster (csrc/hip/graclus.hip)
# ---------------------------------------------------------------------------------------------------

def graclus_cluster(rowptr: Tensor, col: Tensor, weight: Optional[Tensor] = None) -> Tensor:
    """Greedy graph matching in random order (interface of the reference's ``pyg_lib.ops.graclus_cluster``): the nodes of the
    int64 CSR graph ``rowptr`` ``[N + 1]`` / ``col`` ``[E]`` are visited in the order ``torch.randperm(N)`` draws from the
    generator of their device; an unmatched node takes its first unmatched neighbour -- with ``weight`` ``[E]`` the unmatched
    neighbour of the largest weight ``>= 0``, the last one among equals -- and both get the cluster id ``min(u, v)``; a node
    without such a neighbour keeps its own id.  Returns int64 ``[N]``.  See :func:`graclus_cluster_perm`."""
    return torch.ops.pyg.graclus_cluster(rowptr, col, weight)


def graclus_cluster_perm(rowptr: Tensor, col: Tensor, weight: Optional[Tensor], perm: Tensor) -> Tensor:
    """:func:`graclus_cluster` with the visiting order ``perm`` (an int64 permutation of ``0 .. N-1``) given: the deterministic
    core.  HIP and CPU tensors give the same output, on every route.  On a HIP device ``weight`` is float32, float64, float16
    or bfloat16 (the CPU also takes the integer types); the sequential visit is computed exactly in parallel rounds -- one
    launch for graphs of up to 768 nodes and 8 192 entries (capturable into a graph), two launches per round and one stream synchronisation per 16 rounds for
    large ones.  There a ``col`` entry outside ``[0, N)``, a ``rowptr`` outside ``[0, E]`` or a ``perm`` that is no permutation
    touches no memory outside the tensors and is reported by the NEXT graclus call on that device
    (:func:`graclus_pending_error`); on the CPU it raises."""
    return torch.ops.pyg.graclus_cluster_perm(rowptr, col, weight, perm)


def graclus_last_route() -> str:
    """What the last graclus call made from the calling thread on a HIP device ran: ``'<single|multi> r<rounds> b<read-backs>'``
    (test / diagnostic hook; meaningful once the stream has been synchronised; the rule is in include/pyg_hip.h)."""
    return _capi.lib().pyg_hip_graclus_last_route().decode()


@contextlib.contextmanager
def graclus_route(route: Optional[str]):
    """Context manager: the graclus calls of this thread take the ``'single'`` or the ``'multi'`` route whatever their sizes
    (``None``: the library's rule).  For tests and measurements; a forced ``'single'`` call above the capacity of the one
    workgroup (131 072 nodes or 2 097 152 edges) runs ``'multi'``."""
    flags = {None: 0, 'single': 1, 'multi': 2}[route]   # PYG_HIP_GRACLUS_FORCE_*
    prev = _capi.binding().pyg_binding_get_graclus_route()
    _capi.binding().pyg_binding_set_graclus_route(flags)
    try:
        yield
    finally:
        _capi.binding().pyg_binding_set_graclus_route(prev)


def graclus_pending_error() -> int:
    """Returns and clears the word a graclus call on the current HIP device sets when it meets a bad ``col``, ``rowptr`` or
    ``perm`` entry (non-zero: there was one).  Meaningful once the stream has been synchronised."""
    return int(_capi.lib().pyg_hip_graclus_pending_error())


__all__ = [
    'grouped_matmul',
    'segment_matmul',
    'sampled_add',
    'sampled_sub',
    'sampled_mul',
    'sampled_div',
    'fused_scatter_reduce',
    'knn',
    'radius',
    'nearest',
    'fps',
    'grid_cluster',
    'spline_basis',
    'spline_weighting',
    'graclus_cluster',
    'graclus_cluster_perm',
    'index_sort',
    'scatter',
    'scatter_sum',
    'scatter_add',
    'scatter_mul',
    'scatter_mean',
    'scatter_min',
    'scatter_max',
    'scatter_softmax',
    'scatter_log_softmax',
    'scatter_std',
    'scatter_logsumexp',
    'segment_coo',
    'segment_sum_coo',
    'segment_add_coo',
    'segment_mean_coo',
    'segment_min_coo',
    'segment_max_coo',
    'gather_coo',
    'softmax_csr',
    'segment_sum_csr',
    'segment_add_csr',
    'segment_mean_csr',
    'segment_min_csr',
    'segment_max_csr',
    'gather_csr',
    'segment_csr',
]
