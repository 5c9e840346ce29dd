"""Cases of tests/golden/graclus_golden.npz: outputs of the REAL reference's CPU graclus kernel under torch.manual_seed(seed).
Per case the file holds rowptr, col, weight (16-bit floats as their int16 bit patterns), seed, the perm that
torch.randperm(N) gives under that seed, and the reference's output.  The graphs come from tests/_graclus_ref.py."""
import torch

# key, graph family (tests/_graclus_ref.FAMILIES), weight kind, weight dtype, seed
CASES = [
    ('path_none', 'path', 'none', None, 1),
    ('grid_none', 'grid', 'none', None, 2),
    ('random_none', 'random', 'none', None, 3),
    ('decorated_none', 'decorated', 'none', None, 4),
    ('non_symmetric_none', 'non_symmetric', 'none', None, 5),
    ('random_f32', 'random', 'continuous', 'float32', 6),
    ('zipf_f32_ties', 'zipf', 'ties', 'float32', 7),
    ('decorated_f32_special', 'decorated', 'special', 'float32', 8),
    ('grid8_f64', 'grid8', 'continuous', 'float64', 9),
    ('non_symmetric_f64_special', 'decorated_non_symmetric', 'special', 'float64', 10),
    ('star_bf16_ties', 'star', 'ties', 'bfloat16', 11),
    ('random_bf16_special', 'random', 'special', 'bfloat16', 12),
    ('complete_f16', 'complete', 'continuous', 'float16', 13),
    ('zipf_heavy_f16_special', 'zipf_heavy', 'special', 'float16', 14),
    ('random_i64_ties', 'random', 'ties', 'int64', 15),
]
DEVICE_CASES = [c for c in CASES if c[3] != 'int64']   # the device takes the four floating dtypes


def dtype_of(name):
    return None if name is None else getattr(torch, name)


def to_numpy(weight):
    """What the file stores for a weight tensor."""
    return weight.view(torch.int16).numpy() if weight.dtype in (torch.float16, torch.bfloat16) else weight.numpy()


def load(golden, key, dtype_name):
    """(rowptr, col, weight, seed, perm, out) of a case as tensors."""
    rowptr, col = (torch.from_numpy(golden[f'{key}/{n}']) for n in ('rowptr', 'col'))
    weight = None
    if dtype_name is not None:
        weight = torch.from_numpy(golden[f'{key}/weight'])
        if dtype_name in ('float16', 'bfloat16'):
            weight = weight.view(dtype_of(dtype_name))
    return rowptr, col, weight, int(golden[f'{key}/seed']), torch.from_numpy(golden[f'{key}/perm']), torch.from_numpy(golden[f'{key}/out'])
