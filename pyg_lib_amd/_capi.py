"""ctypes view of the C-ABI in include/pyg_hip.h (libpyg_hip.so).

PyTorch is used here only for device memory and the current HIP stream.  There is no CPU
fallback: if the HIP library is missing, importing this module's `lib()` raises.
"""
import ctypes
import os.path as osp

import torch

_HERE = osp.dirname(osp.abspath(__file__))
_LIB = None

OK = 0
ABI_VERSION = 21  # PYG_HIP_ABI_VERSION of the include/pyg_hip.h these bindings were written against
DTYPES = {
    torch.float32: 0,
    torch.float64: 1,
    torch.float16: 2,
    torch.bfloat16: 3,
    torch.int8: 4,
    torch.uint8: 5,
    torch.int16: 6,
    torch.int32: 7,
    torch.int64: 8,
}


class Group(ctypes.Structure):
    """pyg_hip_group"""
    _fields_ = [('input', ctypes.c_void_p), ('other', ctypes.c_void_p), ('out', ctypes.c_void_p),
                ('rows', ctypes.c_int64), ('k', ctypes.c_int32), ('m', ctypes.c_int32),
                ('other_trans', ctypes.c_int32), ('reserved', ctypes.c_int32)]


def lib_path() -> str:
    return osp.join(_HERE, 'libpyg_hip.so')


def lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not osp.exists(path):
            raise ImportError(
                f"pyg_lib_amd: '{path}' not found. Build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = ctypes.CDLL(path)
        c = ctypes
        # a library built from another revision of the header would take `stream` for `flags`: refuse it
        if not hasattr(L, 'pyg_hip_abi_version') or L.pyg_hip_abi_version() != ABI_VERSION:
            got = L.pyg_hip_abi_version() if hasattr(L, 'pyg_hip_abi_version') else '< 5'
            raise ImportError(f"pyg_lib_amd: '{path}' implements C-ABI version {got}, these bindings need {ABI_VERSION}; "
                              f"rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)")
        L.pyg_hip_version.restype = c.c_int64
        L.pyg_hip_last_error.restype = c.c_char_p
        L.pyg_hip_arch.restype = c.c_char_p
        L.pyg_hip_matmul_workspace_size.restype = c.c_size_t
        L.pyg_hip_matmul_workspace_size.argtypes = [c.c_int64]
        L.pyg_hip_matmul_last_variant.restype = c.c_char_p
        L.pyg_hip_scatter_last_route.restype = c.c_char_p
        # (family, dtype, leading, rows, E, K, flags, workspace_bytes, misalign, num_cus)
        L.pyg_hip_csr_route.restype = c.c_char_p
        L.pyg_hip_csr_route.argtypes = [c.c_int, c.c_int] + [c.c_int64] * 4 + [c.c_int, c.c_size_t, c.c_uint, c.c_int]
        L.pyg_hip_csr_last_route.restype = c.c_char_p
        L.pyg_hip_segment_matmul.restype = c.c_int
        L.pyg_hip_segment_matmul.argtypes = [c.c_int, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p,
                                             c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_void_p,
                                             c.c_size_t, c.c_int, c.c_void_p]
        L.pyg_hip_grouped_matmul.restype = c.c_int
        L.pyg_hip_grouped_matmul.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_void_p, c.c_size_t, c.c_int, c.c_void_p]
        L.pyg_hip_set_float_atomic_mode.restype = c.c_int
        L.pyg_hip_set_float_atomic_mode.argtypes = [c.c_int]
        L.pyg_hip_last_accumulate_info.restype = c.c_char_p
        L.pyg_hip_rgcn_pending_error.restype = c.c_int
        # (dtype, K, M, num_relations, flags) -> PYG_HIP_RGCN_ROUTE_*
        L.pyg_hip_rgcn_route.restype = c.c_int
        L.pyg_hip_rgcn_route.argtypes = [c.c_int, c.c_int64, c.c_int64, c.c_int64, c.c_int]
        L.pyg_hip_rgcn_last_route.restype = c.c_char_p
        L.pyg_hip_atomic_selftest.restype = c.c_int
        L.pyg_hip_atomic_selftest.argtypes = [c.c_void_p, c.c_size_t, c.c_int, c.c_char_p, c.c_size_t, c.c_void_p]
        # (fn, dtype, left, left_rows, right, right_rows, index_dtype, left_index, right_index, out, E, F, stream)
        L.pyg_hip_sampled_op.restype = c.c_int
        L.pyg_hip_sampled_op.argtypes = [c.c_int, c.c_int, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int, c.c_void_p,
                                         c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p]
        # (fn, dtype, grad_out, left, left_rows, right, right_rows, index_dtype, left_index, right_index, edge_grad_left,
        #  edge_grad_right, E, F, stream)
        L.pyg_hip_sampled_op_backward.restype = c.c_int
        L.pyg_hip_sampled_op_backward.argtypes = [c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64,
                                                  c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64,
                                                  c.c_int64, c.c_void_p]
        # (dtype, E, N, F)
        L.pyg_hip_fused_scatter_reduce_workspace_size.restype = c.c_size_t
        L.pyg_hip_fused_scatter_reduce_workspace_size.argtypes = [c.c_int, c.c_int64, c.c_int64, c.c_int64]
        # (dtype, src, index, E, F, N, ops, n_ops, out, arg_min, arg_max, count_out, workspace, workspace_bytes, stream)
        L.pyg_hip_fused_scatter_reduce.restype = c.c_int
        L.pyg_hip_fused_scatter_reduce.argtypes = [c.c_int, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64,
                                                   c.POINTER(c.c_int), c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                   c.c_void_p, c.c_size_t, c.c_void_p]
        # (dtype, grad_out, index, arg_min, arg_max, count, E, F, N, ops, n_ops, grad_in, stream)
        L.pyg_hip_fused_scatter_reduce_backward.restype = c.c_int
        L.pyg_hip_fused_scatter_reduce_backward.argtypes = [c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                            c.c_int64, c.c_int64, c.c_int64, c.POINTER(c.c_int), c.c_int,
                                                            c.c_void_p, c.c_void_p]
        # knn / radius / nearest (include/pyg_hip.h, "knn, radius, nearest"); x, y are (pointer, rows) pairs
        L.pyg_hip_spatial_route.restype = c.c_int
        L.pyg_hip_spatial_route.argtypes = [c.c_int, c.c_int, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int64]
        L.pyg_hip_spatial_last_route.restype = c.c_char_p
        L.pyg_hip_spatial_tile.restype = c.c_int
        L.pyg_hip_spatial_tile.argtypes = [c.c_int]
        # (op, dtype, M, N, B, D, k, flags)
        L.pyg_hip_spatial_workspace_size.restype = c.c_size_t
        L.pyg_hip_spatial_workspace_size.argtypes = [c.c_int, c.c_int, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int]
        # (dtype, x, N, y, M, D, ptr_x, ptr_y, num_examples, k, flags, workspace, workspace_bytes, num_pairs, stream)
        L.pyg_hip_knn.restype = c.c_int
        L.pyg_hip_knn.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p,
                                  c.c_int64, c.c_int64, c.c_int, c.c_void_p, c.c_size_t, c.POINTER(c.c_int64), c.c_void_p]
        # (dtype, N, M, D, num_examples, k, flags, workspace, workspace_bytes, num_pairs, out, stream)
        L.pyg_hip_knn_emit.restype = c.c_int
        L.pyg_hip_knn_emit.argtypes = [c.c_int, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int, c.c_void_p,
                                       c.c_size_t, c.c_int64, c.c_void_p, c.c_void_p]
        # (dtype, x, N, y, M, D, ptr_x, ptr_y, num_examples, r, max_num_neighbors, flags, workspace, workspace_bytes, num_pairs, stream)
        L.pyg_hip_radius.restype = c.c_int
        L.pyg_hip_radius.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p,
                                     c.c_int64, c.c_double, c.c_int64, c.c_int, c.c_void_p, c.c_size_t, c.POINTER(c.c_int64),
                                     c.c_void_p]
        # (... as pyg_hip_radius up to workspace_bytes, num_pairs, out, stream)
        L.pyg_hip_radius_emit.restype = c.c_int
        L.pyg_hip_radius_emit.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p,
                                          c.c_int64, c.c_double, c.c_int64, c.c_int, c.c_void_p, c.c_size_t, c.c_int64,
                                          c.c_void_p, c.c_void_p]
        # (dtype, x, N, y, M, D, ptr_x, ptr_y, num_examples, flags, workspace, workspace_bytes, out, stream)
        L.pyg_hip_nearest.restype = c.c_int
        L.pyg_hip_nearest.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p,
                                      c.c_int64, c.c_int, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
        L.pyg_hip_nearest_pending_error.restype = c.c_int
        # fps / grid_cluster (include/pyg_hip.h, "fps, grid_cluster")
        # (dtype, B, D, max_points, max_samples, flags)
        L.pyg_hip_fps_route.restype = c.c_int
        L.pyg_hip_fps_route.argtypes = [c.c_int, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int]
        L.pyg_hip_fps_last_route.restype = c.c_char_p
        L.pyg_hip_fps_tile.restype = c.c_int
        L.pyg_hip_fps_tile.argtypes = [c.c_int]
        # (dtype, N, B, D, max_points, max_samples, flags)
        L.pyg_hip_fps_workspace_size.restype = c.c_size_t
        L.pyg_hip_fps_workspace_size.argtypes = [c.c_int, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int]
        # (dtype, src, N, D, ptr, B, out_ptr, start, max_points, max_samples, flags, workspace, workspace_bytes, out, out_total, stream)
        L.pyg_hip_fps.restype = c.c_int
        L.pyg_hip_fps.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p,
                                  c.c_int64, c.c_int64, c.c_int, c.c_void_p, c.c_size_t, c.c_void_p, c.c_int64, c.c_void_p]
        L.pyg_hip_fps_pending_error.restype = c.c_int
        # (dtype, N, D, have_start, have_end)
        L.pyg_hip_grid_cluster_workspace_size.restype = c.c_size_t
        L.pyg_hip_grid_cluster_workspace_size.argtypes = [c.c_int, c.c_int64, c.c_int64, c.c_int, c.c_int]
        # (dtype, pos, N, D, size, start, end, workspace, workspace_bytes, out, stream)
        L.pyg_hip_grid_cluster.restype = c.c_int
        L.pyg_hip_grid_cluster.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                           c.c_size_t, c.c_void_p, c.c_void_p]
        # spline_basis / spline_weighting (include/pyg_hip.h, "spline_basis, spline_weighting")
        # (dtype, E, S, M_in, M_out, K)
        L.pyg_hip_spline_route.restype = c.c_int
        L.pyg_hip_spline_route.argtypes = [c.c_int] + [c.c_int64] * 5
        L.pyg_hip_spline_last_route.restype = c.c_char_p
        L.pyg_hip_spline_tile.restype = c.c_int
        L.pyg_hip_spline_tile.argtypes = [c.c_int]
        L.pyg_hip_spline_pending_error.restype = c.c_int
        # (dtype, pseudo, kernel_size, is_open_spline, E, D, degree, basis, weight_index, stream)
        L.pyg_hip_spline_basis.restype = c.c_int
        L.pyg_hip_spline_basis.argtypes = [c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int, c.c_void_p,
                                           c.c_void_p, c.c_void_p]
        # (dtype, grad_basis, pseudo, kernel_size, is_open_spline, E, D, S, degree, grad_pseudo, stream)
        L.pyg_hip_spline_basis_backward.restype = c.c_int
        L.pyg_hip_spline_basis_backward.argtypes = [c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64,
                                                    c.c_int64, c.c_int, c.c_void_p, c.c_void_p]
        # (dtype, x, weight, basis, weight_index, E, S, M_in, M_out, K, flags, out, stream)
        L.pyg_hip_spline_weighting.restype = c.c_int
        L.pyg_hip_spline_weighting.argtypes = [c.c_int] + [c.c_void_p] * 4 + [c.c_int64] * 5 + [c.c_int, c.c_void_p, c.c_void_p]
        # (dtype, grad_out, x, weight, weight_index, E, S, M_in, M_out, K, flags, grad_basis, stream)
        L.pyg_hip_spline_weighting_backward_basis.restype = c.c_int
        L.pyg_hip_spline_weighting_backward_basis.argtypes = L.pyg_hip_spline_weighting.argtypes
        # (dtype, M_in, M_out, K)
        L.pyg_hip_spline_backward_x_workspace_size.restype = c.c_size_t
        L.pyg_hip_spline_backward_x_workspace_size.argtypes = [c.c_int, c.c_int64, c.c_int64, c.c_int64]
        # (dtype, grad_out, weight, basis, weight_index, E, S, M_in, M_out, K, flags, workspace, workspace_bytes, grad_x, stream)
        L.pyg_hip_spline_weighting_backward_x.restype = c.c_int
        L.pyg_hip_spline_weighting_backward_x.argtypes = [c.c_int] + [c.c_void_p] * 4 + [c.c_int64] * 5 + [c.c_int, c.c_void_p, c.c_size_t,
                                                                                                        c.c_void_p, c.c_void_p]
        # (dtype, E, S, M_in, M_out, K, flags)
        L.pyg_hip_spline_backward_weight_workspace_size.restype = c.c_size_t
        L.pyg_hip_spline_backward_weight_workspace_size.argtypes = [c.c_int] + [c.c_int64] * 5 + [c.c_int]
        # (dtype, grad_out, x, basis, weight_index, E, S, M_in, M_out, K, flags, workspace, workspace_bytes, grad_weight, stream)
        L.pyg_hip_spline_weighting_backward_weight.restype = c.c_int
        L.pyg_hip_spline_weighting_backward_weight.argtypes = L.pyg_hip_spline_weighting_backward_x.argtypes
        # graclus_cluster (include/pyg_hip.h, "graclus_cluster")
        # (N, E, flags)
        L.pyg_hip_graclus_route.restype = c.c_int
        L.pyg_hip_graclus_route.argtypes = [c.c_int64, c.c_int64, c.c_int]
        L.pyg_hip_graclus_last_route.restype = c.c_char_p
        L.pyg_hip_graclus_tile.restype = c.c_int
        L.pyg_hip_graclus_tile.argtypes = [c.c_int]
        L.pyg_hip_graclus_workspace_size.restype = c.c_size_t
        L.pyg_hip_graclus_workspace_size.argtypes = [c.c_int64, c.c_int64, c.c_int]
        # (rowptr, col, weight_dtype, weight, perm, N, E, flags, workspace, workspace_bytes, out, stream)
        L.pyg_hip_graclus.restype = c.c_int
        L.pyg_hip_graclus.argtypes = [c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int,
                                      c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
        L.pyg_hip_graclus_pending_error.restype = c.c_int
        # node2vec_walk (include/pyg_hip.h, "node2vec walks")
        # (index_dtype, rowptr, N, col, E, seed, S, L, a_ret, a_near, a_far, key, max_attempts, out, stream)
        L.pyg_hip_node2vec_walk.restype = c.c_int
        L.pyg_hip_node2vec_walk.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64,
                                            c.c_float, c.c_float, c.c_float, c.c_uint64, c.c_int, c.c_void_p, c.c_void_p]
        # edge_lookup / negative_sample (include/pyg_hip.h, "Edge lookup and negative sampling"); src and ptr may be NULL
        # (index_dtype, rowptr, num_src, col, num_edges, src, dst, num_queries, out, stream)
        L.pyg_hip_edge_lookup.restype = c.c_int
        L.pyg_hip_edge_lookup.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p, c.c_int64,
                                          c.c_void_p, c.c_void_p]
        # (index_dtype, rowptr, num_src, col, num_edges, src, num_items, num_dst, num_neg, key, exclude_self, ptr, num_graphs,
        #  out, stream)
        L.pyg_hip_negative_sample.restype = c.c_int
        L.pyg_hip_negative_sample.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64,
                                              c.c_int64, c.c_int64, c.c_uint64, c.c_int, c.c_void_p, c.c_int64, c.c_void_p,
                                              c.c_void_p]
        _LIB = L
    return _LIB


_BINDING = None


def binding() -> ctypes.CDLL:
    """libpyg.so (the torch operator library) through ctypes, for its two non-operator hooks."""
    global _BINDING
    if _BINDING is None:
        L = ctypes.CDLL(osp.join(_HERE, 'libpyg.so'))
        L.pyg_binding_set_matmul_schedule.restype = None
        L.pyg_binding_set_matmul_schedule.argtypes = [ctypes.c_int]
        L.pyg_binding_get_matmul_schedule.restype = ctypes.c_int
        L.pyg_binding_set_spatial_route.restype = None
        L.pyg_binding_set_spatial_route.argtypes = [ctypes.c_int]
        L.pyg_binding_get_spatial_route.restype = ctypes.c_int
        L.pyg_binding_set_fps_route.restype = None
        L.pyg_binding_set_fps_route.argtypes = [ctypes.c_int]
        L.pyg_binding_get_fps_route.restype = ctypes.c_int
        L.pyg_binding_set_spline_route.restype = None
        L.pyg_binding_set_spline_route.argtypes = [ctypes.c_int]
        L.pyg_binding_get_spline_route.restype = ctypes.c_int
        L.pyg_binding_set_graclus_route.restype = None
        L.pyg_binding_set_graclus_route.argtypes = [ctypes.c_int]
        L.pyg_binding_get_graclus_route.restype = ctypes.c_int
        _BINDING = L
    return _BINDING


def check(rc: int) -> None:
    if rc != OK:
        raise RuntimeError(lib().pyg_hip_last_error().decode())


def stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"pyg_lib_amd: '{name}' must live on a HIP device (got {t.device}); this build has no CPU path")
