"""What the row hooks' test classes share (tests/_bsdf_common.py, _light_common.py, _interaction_common.py, _texture_common.py): rows of floats go
to a hook of either backend, rows of floats come back."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

f32 = np.float32


def run_rows(be, call, rows, width_in, width_out):
    """call(rows pointer, n, output pointer) -> status over `rows` as [n, width_in] float32; -> [n, width_out] float32.  Every status goes
    through be.check.  The oracle walks the rows on the calling thread: from 65536 rows on they are split over eight threads for it."""
    rows = np.ascontiguousarray(rows, f32).reshape(-1, width_in)
    n = rows.shape[0]
    out = np.empty((n, width_out), f32)

    def part(lo, hi):
        return call(rows[lo:hi].ctypes.data_as(C.c_void_p), hi - lo, out[lo:hi].ctypes.data_as(C.c_void_p))
    if be.is_oracle and n >= 65536:
        cuts = np.linspace(0, n, 9).astype(int)
        with ThreadPoolExecutor(8) as ex:
            rcs = list(ex.map(lambda k: part(cuts[k], cuts[k + 1]), range(8)))
    else:
        rcs = [part(0, n)]
    for rc in rcs:
        be.check(rc)
    return out
