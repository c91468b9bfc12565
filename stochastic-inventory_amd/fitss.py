"""sdp.inventory.FitsS (FitsS.java:21-292): fit a one-, two- or three-level (s, S) rule to the optimal table of a
capacitated lot-sizing recursion -- the step the capacitated.fitss drivers take after every solve
(ThreeLevelFitsSTest.java:137-139).  Same names and argument meaning as the reference; every method sits on the library's
host entry points (sdpgpu_fit_ss, sdpgpu_fit_level_index, sdpgpu_fit_min_square; include/sdpgpu.h), which need no device,
so the table may come from `Recursion.getOptTable()`, `RecursionBatch.getOptTable(i)` or anywhere else.

`minSquare` is the closed form of the one-variable problem the reference hands to CPLEX: the mean of the terms,
clamped to [lb, 10000].  The fit of a whole solved batch runs on the device instead: `SdpBatch.fit_ss(levels)`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import SdpgpuError
from .engine import _dp, _ip


def _rows(table) -> np.ndarray:
    rows = np.ascontiguousarray(table, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != 3:
        raise ValueError(f"opt table of shape {rows.shape}: expected rows [period, inventory, quantity]")
    return rows


class FitsS:
    def __init__(self, maxOrderQuantity: int, T: int):
        self.maxOrderQuantity = int(maxOrderQuantity)  # (an int field in the reference, FitsS.java:23)
        self.T = int(T)
        self._lib = _abi.load()

    def _check(self, rc: int):
        if rc:
            raise SdpgpuError(rc, self._lib.sdpgpu_last_error(None).decode())

    def levelIndex(self, optTable) -> np.ndarray:
        """FitsS.java:39-59 on the rows of ONE period."""
        rows = _rows(optTable)
        q = np.ascontiguousarray(rows[:, 2])
        out = np.empty(max(len(q), 1), dtype=np.int32)
        n = C.c_int32()
        self._check(self._lib.sdpgpu_fit_level_index(float(self.maxOrderQuantity), _dp(q), len(q), _ip(out), C.byref(n)))
        return out[:n.value].copy()

    def minSquare(self, lb: float, upIndex: int, tOptTable) -> float:
        """FitsS.java:69-98 on the rows of ONE period, in closed form."""
        rows = _rows(tOptTable)
        x, q = np.ascontiguousarray(rows[:, 1]), np.ascontiguousarray(rows[:, 2])
        out = C.c_double()
        self._check(self._lib.sdpgpu_fit_min_square(float(self.maxOrderQuantity), float(lb), int(upIndex), _dp(x), _dp(q), len(x),
                                                    C.byref(out)))
        return float(out.value)

    def _fit(self, levels: int, optimalTable) -> np.ndarray:
        rows = _rows(optimalTable)
        out = np.empty((self.T, 2 * levels), dtype=np.float64)
        self._check(self._lib.sdpgpu_fit_ss(levels, self.T, float(self.maxOrderQuantity), _dp(rows), len(rows), _dp(out)))
        return out

    def getSinglesS(self, optimalTable) -> np.ndarray:
        """FitsS.java:100-130: [T, 2] = (s, S) per period."""
        return self._fit(1, optimalTable)

    def getOnlySinglesS(self, optimalTable) -> np.ndarray:
        """FitsS.java:132-153: getSinglesS where a period's levelIndex has ONE entry that is not row 0; any other period
        stays (0, 0) and the reference prints "may be wrong!"."""
        rows = _rows(optimalTable)
        out = self._fit(1, rows)
        for t in range(1, self.T):
            idx = self.levelIndex(rows[rows[:, 0] == t + 1])
            if not (len(idx) == 1 and idx[0] != 0):
                print("may be wrong!")
                out[t] = 0.0
        return out

    def getTwosS(self, optimalTable) -> np.ndarray:
        """FitsS.java:155-211: [T, 4] = (s1, S1, s2, S2) per period."""
        return self._fit(2, optimalTable)

    def getThreesS(self, optimalTable) -> np.ndarray:
        """FitsS.java:213-291: [T, 6] = (s1, S1, s2, S2, s3, S3) per period."""
        return self._fit(3, optimalTable)


class FindsSOverDraft:
    """cash.overdraft.FindsSOverDraft(T, iniCash) (FindsSOverDraft.java:20-103): the (s, S) and (s, C, S) rules the overdraft
    drivers read off CashRecursion.getOptTable() -- rows [period, x, cash, Q], sorted as the reference's TreeMap sorts its keys --
    before they roll them out (CashSimulation.simulatesSOD / simulatesCSDraft).  Host only, a few passes over the table.  The
    reference's loops verbatim, including the read of row j + 1 where the LAST row of a period orders (an
    ArrayIndexOutOfBoundsException there, an IndexError here) and the `cash + Q` on the left of getsCS's comparison (:86).
    getsCS1S2 is not mirrored: its rule arrives as an array (CashSimulation.simulatesSOD2)."""

    def __init__(self, T: int, iniCash: float):
        self.T = int(T)
        self.iniCash = float(iniCash)

    @staticmethod
    def _table(optimalTable) -> np.ndarray:
        rows = np.asarray(optimalTable, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] < 4 or len(rows) == 0:
            raise ValueError(f"optimalTable of shape {rows.shape}: rows [period, x, cash, Q]")
        return rows

    def getsS(self, optimalTable) -> np.ndarray:
        """:35-55: s = the inventory of the row AFTER the last ordering row of the period, S = that row's x + Q."""
        tab = self._table(optimalTable)
        out = np.zeros((self.T, 2))
        out[0, 0] = tab[0, 1]
        out[0, 1] = tab[0, 1] + tab[0, 3]
        for t in range(1, self.T):
            rows = tab[tab[:, 0] == t + 1]
            for j in range(len(rows) - 1, -1, -1):
                if rows[j, 3] != 0:
                    if j + 1 >= len(rows):
                        raise IndexError(f"getsS: the last row of period {t + 1} orders; tOptTable[j + 1] does not exist")
                    out[t, 0] = rows[j + 1, 1]
                    out[t, 1] = rows[j, 1] + rows[j, 3]
                    break
        return out

    def getsCS(self, optimalTable) -> np.ndarray:
        """:62-103: s as getsS; S = x + Q of the ordering rows that pass `cash + Q > S so far`; C = the largest cash of a
        non-ordering row below an ordering one (from -500)."""
        tab = self._table(optimalTable)
        out = np.zeros((self.T, 3))
        minCashUsed = -500.0
        out[0, 0] = tab[0, 1]
        out[0, 1] = tab[0, 2]
        out[0, 2] = tab[0, 1] + tab[0, 3]
        for t in range(1, self.T):
            rows = tab[tab[:, 0] == t + 1]
            recordsTime = 0
            out[t, 2] = 0.0
            out[t, 1] = minCashUsed
            mark_s = 0
            for j in range(len(rows) - 1, -1, -1):
                if rows[j, 3] != 0:
                    if mark_s == 0:
                        if j + 1 >= len(rows):
                            raise IndexError(f"getsCS: the last row of period {t + 1} orders; tOptTable[j + 1] does not exist")
                        out[t, 0] = rows[j + 1, 1]
                        mark_s = 1
                    if rows[j, 2] + rows[j, 3] > out[t, 2]:
                        out[t, 2] = rows[j, 1] + rows[j, 3]
                    recordsTime = 1
                if rows[j, 3] == 0 and recordsTime == 1:
                    if rows[j, 2] > out[t, 1]:
                        out[t, 1] = rows[j, 2]
        return out
