"""sdp.inventory.CheckKConvexity (CheckKConvexity.java:4-69): the structure checks the reference's drivers run on a row of
values after a solve -- `check` (K-convexity, :39-68; CLSPforDraw.java:181-182, WorkforcePlanning.java:208-209) and `checkCK`
(CK-convexity of Gallego and Scheller-Wolf 2000, :6-36; ThreeLevelFitsSTest.java:159).  Same names, arguments and return
values as the reference; both sit on the library's host entry point (sdpgpu_check_convexity, include/sdpgpu.h), which needs
no device, so `yG` may come from anywhere.  Every instance of a solved batch is checked on the device instead:
`SdpBatch.check_convexity`, `RecursionBatch.checkKConvexity` / `checkCK`.

`yG` is the reference's `double[n][2]`: column 0 the abscissae (unit-spaced in every caller, so xLength = n), column 1 the
values.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import SdpgpuConvexity, SdpgpuError
from .engine import _dp

CHECK, CHECK_CK = 0, 1
CONVEXITY_DTYPE = np.dtype([("holds", np.int32), ("i0", np.int32), ("i1", np.int32), ("i2", np.int32), ("lhs", np.float64),
                            ("rhs", np.float64)])
CK_HOLDS, CK_FAILS = "CK convexity holds", "not CK convex"


def check_row(kind: int, g, K: float, capacity: int = 0) -> SdpgpuConvexity:
    """sdpgpu_check_convexity on one row of values: the struct of the first violating triple, or holds = 1."""
    lib = _abi.load()
    row = np.ascontiguousarray(g, dtype=np.float64)
    if row.ndim != 1:
        raise ValueError(f"a row of shape {row.shape}: expected one dimension")
    out = SdpgpuConvexity()
    rc = lib.sdpgpu_check_convexity(int(kind), _dp(row) if len(row) else None, len(row), float(K), int(capacity), C.byref(out))
    if rc:
        raise SdpgpuError(rc, lib.sdpgpu_batch_last_error(None).decode())
    return out


def _values(yG) -> np.ndarray:
    rows = np.ascontiguousarray(yG, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != 2:
        raise ValueError(f"yG of shape {rows.shape}: expected rows [y, G(y)]")
    if len(rows) and int(rows[-1, 0] - rows[0, 0] + 1) != len(rows):
        raise ValueError(f"yG spans {rows[0, 0]} .. {rows[-1, 0]} in {len(rows)} rows: the check takes its length from the "
                         "abscissae (CheckKConvexity.java:9), which is the row count for unit-spaced rows only")
    return np.ascontiguousarray(rows[:, 1])


class CheckKConvexity:
    @staticmethod
    def checkCK(yG, fixOrderCost: float, capacity: int) -> str:
        """CheckKConvexity.java:6-36: "CK convexity holds" or "not CK convex", with the reference's printed lines."""
        r = check_row(CHECK_CK, _values(yG), fixOrderCost, capacity)
        if r.holds:
            print(CK_HOLDS)
            return CK_HOLDS
        rows = np.asarray(yG, dtype=np.float64)
        print(r.lhs)
        print(r.rhs)
        print("z = %d, y = %d, b = %d" % (int(rows[r.i1, 0]), int(rows[r.i0, 0]), int(rows[r.i2, 0])))
        print(CK_FAILS)
        return CK_FAILS

    @staticmethod
    def check(yG, fixOrderCost: float) -> bool:
        """CheckKConvexity.java:39-68: True iff K-convexity holds, with the reference's printed lines."""
        r = check_row(CHECK, _values(yG), fixOrderCost)
        if r.holds:
            print("K convexity holds")
            return True
        rows = np.asarray(yG, dtype=np.float64)
        print(r.lhs)
        print(r.rhs)
        print("x-b = %d, x = %d, x+a = %d" % (int(rows[r.i2, 0]), int(rows[r.i1, 0]), int(rows[r.i0, 0])))
        print("not K convex")
        return False
