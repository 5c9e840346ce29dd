"""A fixture `<name>` is stored as `<name>.part<i>.npz` files, each under 1 MiB (the limit for a committed file): whole
arrays, in key order, compressed as np.savez_compressed does.  `load` returns all arrays of the fixture as one dict."""
import glob
import io
import os
import os.path as osp
import re
import zipfile

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
PART_LIMIT = 960 * 1024


def part_files(name):
    files = glob.glob(osp.join(HERE, name + '.part*.npz'))
    return sorted(files, key=lambda f: int(re.search(r'\.part(\d+)\.npz$', f).group(1)))


def load(name):
    files = part_files(name)
    if not files:
        raise FileNotFoundError(f'no {name}.part*.npz under {HERE}')
    out = {}
    for f in files:
        with np.load(f) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _zip(members):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for key, raw in members:
            # a fixed time stamp: the same arrays give the same bytes whenever the generator runs
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, raw)
    return buf.getvalue()


def save(name, arrays):
    """Stores what np.savez_compressed(<name>.npz, **arrays) would, as parts (replacing the old ones); returns the
    number of parts."""
    for f in part_files(name):
        os.remove(f)
    parts, cur, size = [], [], 0
    for key, a in arrays.items():
        buf = io.BytesIO()
        np.save(buf, np.asanyarray(a), allow_pickle=False)
        member = (key, buf.getvalue())
        csize = len(_zip([member]))
        if cur and size + csize > PART_LIMIT:
            parts.append(cur)
            cur, size = [], 0
        cur.append(member)
        size += csize
    if cur:
        parts.append(cur)
    for i, p in enumerate(parts):
        data = _zip(p)
        assert len(data) < 1 << 20, f'{name}: one array compresses to {len(data)} bytes'
        with open(osp.join(HERE, f'{name}.part{i}.npz'), 'wb') as f:
            f.write(data)
    return len(parts)
