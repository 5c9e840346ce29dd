"""One way to record a call into a HIP graph and to replay it on other data (tests/test_graph_replay_gpu.py).

`capture(fn)` follows tests/test_fused_reduce_gpu.py::test_forward_and_backward_replay_from_a_captured_graph: two warm-up
calls on a side stream (kernel attributes, allocator pools, the autograd threads), with the waits on both sides, a device
synchronisation, then the call under `torch.cuda.graph`.  `replays(...)` writes every variant's tensors into the static
inputs, replays, and issues the same call eagerly on fresh copies of the same tensors; the test compares the two results
with each other and with its own reference.

One process, one stream; nothing here changes how the runtime replays a graph.  Not a conftest: the module is imported by
the tests that use it.
"""
import torch


def warm_up(fn, times: int = 2):
    """What has to happen before ANY capture: `fn()` eagerly on a side stream, with the waits on both sides, then a device
    synchronisation.  Everything lazy happens here and not under capture -- code objects are loaded at a kernel's first
    launch, kernel attributes are set, the allocator's pools grow, the autograd engine starts its device threads at the
    first backward of the process."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())   # the inputs are produced on the current stream
    with torch.cuda.stream(side):
        for _ in range(times):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def capture(fn, warmup: int = 2):
    """Record `fn()` -- a call on static tensors that returns a tensor or a tuple of tensors.  Returns (graph, outputs):
    the outputs are static too, every replay overwrites them."""
    warm_up(fn, warmup)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = fn()
    return graph, _as_tuple(outs)


def _as_tuple(outs):
    return tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)


def fresh(tensors: dict, like: dict, device) -> dict:
    """Fresh device copies of the CPU tensors of a variant; a copy requires grad where the static tensor `like[name]` does."""
    return {k: v.to(device).requires_grad_(like[k].requires_grad) for k, v in tensors.items()}


def replays(graph, static_in: dict, static_out: tuple, variants, eager, after_replay=None):
    """For every (name, tensors) of `variants` -- `tensors` maps the names of `static_in` to CPU tensors of the same shape and
    dtype --: copy into the static inputs, replay, synchronise, clone the static outputs; then `eager(inputs)` on fresh
    copies.  Yields (name, tensors, replayed outputs, eager outputs).  `after_replay(name)` runs between the replay and the
    eager call (guard checks)."""
    device = next(iter(static_in.values())).device
    for name, tensors in variants:
        assert set(tensors) == set(static_in), (name, sorted(tensors), sorted(static_in))
        with torch.no_grad():
            for k, v in tensors.items():
                assert v.shape == static_in[k].shape and v.dtype == static_in[k].dtype, (name, k)
                static_in[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        got = tuple(o.detach().clone() for o in static_out)
        if after_replay is not None:
            after_replay(name)
        want = _as_tuple(eager(fresh(tensors, static_in, device)))
        torch.cuda.synchronize()
        yield name, tensors, got, tuple(o.detach() for o in want)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit equality (NaN payloads and the sign of zero included)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(view).cpu(), b.contiguous().view(view).cpu())
