"""The structure tables of the cash drivers and their checks (sdpgpu_cash_structure / sdpgpu_cash_structure_host,
include/sdpgpu.h; DESIGN 4, "Cash structure tables"): sdp.cash.CashRecursion's getH, getMinusGAGB, getMinusFG,
checkSingleCrossing, checkNonIncreasing and checkNonDecreasing (CashRecursion.java:227-404) on tables G, GA, GB, F.

`run(...)` is the one call both routes go through: `host=True` is the library's plain loops on the caller's tables (no
device), otherwise the kernels -- on the caller's tables (`source = 1`, a handle is optional) or on the tables of a solved
handle, formed on the device (`source = 0`).  getH3Column is done here, from H and G.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

from . import _abi
from ._abi import SdpgpuCashStructureIn, SdpgpuCashStructureOut, SdpgpuError
from .engine import _dp, _ip

SLOT = {"h": 0, "gagb": 1, "fg": 2}
SOURCE_NAMES = ("g", "ga", "gb", "f")


def mask_of(tables=(), single_crossing=False, non_increasing=(), non_decreasing=()) -> int:
    """The request mask from names: tables / non_increasing / non_decreasing are iterables of "h", "gagb", "fg"."""
    m = 0
    for t in tables:
        m |= 1 << SLOT[t]
    if single_crossing:
        m |= _abi.CSTRUCT_SINGLE_CROSS
    for t in non_increasing:
        m |= _abi.CSTRUCT_NONINC(SLOT[t])
    for t in non_decreasing:
        m |= _abi.CSTRUCT_NONDEC(SLOT[t])
    return m


def tables_of_mask(mask: int, given=()):
    """-> (source tables read, derived tables taking part) by name, as the library decides them; `given`: the derived
    tables the caller hands over instead of having them formed."""
    tab = [bool(mask & (1 << s)) or bool(mask & _abi.CSTRUCT_NONINC(s)) or bool(mask & _abi.CSTRUCT_NONDEC(s)) for s in range(3)]
    tab[0] = tab[0] or bool(mask & _abi.CSTRUCT_SINGLE_CROSS)
    formed = [tab[s] and name not in given for name, s in SLOT.items()]
    src = {"g": formed[0] or formed[2], "ga": formed[1], "gb": formed[1], "f": formed[2]}
    return [n for n in SOURCE_NAMES if src[n]], [n for n in SLOT if tab[SLOT[n]]]


@dataclass
class CashStructure:
    """What one call returns: the tables it formed or read (by name: g, ga, gb, f, h, opt_y, gagb, fg), the verdicts as
    (holds, i, j, i1, j1, value) tuples keyed "single_crossing", "non_increasing:<table>", "non_decreasing:<table>", and the
    kernels' HIP-event time (0.0 from the host route)."""
    tables: Dict[str, Optional[np.ndarray]] = field(default_factory=dict)
    verdicts: Dict[str, tuple] = field(default_factory=dict)
    kernel_ms: float = 0.0

    def __getattr__(self, name):
        tabs = self.__dict__.get("tables", {})
        if name in tabs:
            return tabs[name]
        raise AttributeError(name)

    def holds(self, key: str) -> bool:
        return bool(self.verdicts[key][0])


def run(mask: int, *, n_r: int, n_x: int, min_cash: float, fix_cost: float, vari_cost: float, source: int = 1, handle=None,
        host: bool = False, device: int = -1, period: int = 1, x_lo: float = 0.0, g=None, ga=None, gb=None, f=None, h=None,
        gagb=None, fg=None, want_tables: bool = True) -> CashStructure:
    lib = _abi.load()
    inp = SdpgpuCashStructureIn()
    inp.source, inp.mask, inp.device, inp.period = int(source), int(mask), int(device), int(period)
    inp.n_r, inp.n_x = int(n_r), int(n_x)
    inp.x_lo, inp.min_cash, inp.fix_cost, inp.vari_cost = float(x_lo), float(min_cash), float(fix_cost), float(vari_cost)
    keep, given = [], []
    for name, arr in zip(SOURCE_NAMES + tuple(SLOT), (g, ga, gb, f, h, gagb, fg)):
        if arr is None:
            continue
        a = np.ascontiguousarray(arr, dtype=np.float64)
        if a.shape != (inp.n_r, inp.n_x):
            raise ValueError(f"table {name} of shape {a.shape}: expected ({inp.n_r}, {inp.n_x})")
        keep.append(a)
        setattr(inp, name, _dp(a))
        if name in SLOT and inp.source == 1:
            given.append(name)
    out = SdpgpuCashStructureOut()
    res = CashStructure()
    sized = 1 <= inp.n_r <= _abi.CSTRUCT_MAX_AXIS and 1 <= inp.n_x <= _abi.CSTRUCT_MAX_AXIS
    if want_tables and sized and 1 <= inp.mask <= _abi.CSTRUCT_ALL:
        src_names, tab_names = tables_of_mask(inp.mask, given)
        for name in src_names + tab_names:
            res.tables[name] = np.empty((inp.n_r, inp.n_x), dtype=np.float64)
            setattr(out, name, _dp(res.tables[name]))
        if "h" in tab_names and "h" not in given:
            res.tables["opt_y"] = np.empty((inp.n_r, inp.n_x), dtype=np.int32)
            out.opt_y = _ip(res.tables["opt_y"])
    if host:
        rc = lib.sdpgpu_cash_structure_host(C.byref(inp), C.byref(out))
        handle = None
    else:
        rc = lib.sdpgpu_cash_structure(handle, C.byref(inp), C.byref(out))
    if rc:
        raise SdpgpuError(rc, lib.sdpgpu_last_error(handle).decode())
    if inp.mask & _abi.CSTRUCT_SINGLE_CROSS:
        res.verdicts["single_crossing"] = out.single_crossing.as_tuple()
    for name, s in SLOT.items():
        if inp.mask & _abi.CSTRUCT_NONINC(s):
            res.verdicts["non_increasing:" + name] = out.non_increasing[s].as_tuple()
        if inp.mask & _abi.CSTRUCT_NONDEC(s):
            res.verdicts["non_decreasing:" + name] = out.non_decreasing[s].as_tuple()
    res.kernel_ms = float(out.kernel_ms)
    return res


def _table(arr) -> np.ndarray:
    a = np.ascontiguousarray(arr, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"a table of shape {a.shape}: expected double[RLength][xLength]")
    return a


def check_table(check: str, arr, *, host: bool = True, handle=None, device: int = -1) -> tuple:
    """One of the reference's three checks ("single_crossing", "non_increasing", "non_decreasing") on a table the caller
    holds, handed over as the H slot: the verdict tuple (holds, i, j, i1, j1, value)."""
    a = _table(arr)
    mask = {"single_crossing": _abi.CSTRUCT_SINGLE_CROSS, "non_increasing": _abi.CSTRUCT_NONINC(0),
            "non_decreasing": _abi.CSTRUCT_NONDEC(0)}[check]
    r = run(mask, n_r=a.shape[0], n_x=a.shape[1], min_cash=0.0, fix_cost=0.0, vari_cost=1.0, h=a, host=host, handle=handle,
            device=device, want_tables=False)
    return next(iter(r.verdicts.values()))


class CashStructureMethods:
    """sdp.cash.CashRecursion's table methods with the reference's names, arguments and return shapes
    (CashRecursion.java:227-404).  They sit on the host entry point and need no device, so the tables may come from
    anywhere -- a G table this class drew, `GA.csv` written earlier, hand-built rows."""

    @staticmethod
    def getMinusGAGB(resultGA, resultGB, minCash, fixCost, variCost) -> np.ndarray:
        ga, gb = _table(resultGA), _table(resultGB)
        return run(mask_of(["gagb"]), n_r=ga.shape[0], n_x=ga.shape[1], min_cash=minCash, fix_cost=fixCost, vari_cost=variCost, ga=ga,
                   gb=gb, host=True).gagb

    @staticmethod
    def getMinusFG(resultG, resultF, minCash, fixCost, variCost) -> np.ndarray:
        g, f = _table(resultG), _table(resultF)
        return run(mask_of(["fg"]), n_r=g.shape[0], n_x=g.shape[1], min_cash=minCash, fix_cost=fixCost, vari_cost=variCost, g=g, f=f,
                   host=True).fg

    @staticmethod
    def getH(resultG, minCash, fixCost, variCost) -> np.ndarray:
        g = _table(resultG)
        return run(mask_of(["h"]), n_r=g.shape[0], n_x=g.shape[1], min_cash=minCash, fix_cost=fixCost, vari_cost=variCost, g=g, host=True).h

    @staticmethod
    def getH3Column(resultG, minCash, fixCost, variCost) -> np.ndarray:
        """CashRecursion.java:327-356: rows [resultG[i][0], resultG[0][j], H[i][j]], i outer -- the first two columns are
        the reference's (entries of G, not the abscissae)."""
        g = _table(resultG)
        h = CashStructureMethods.getH(g, minCash, fixCost, variCost)
        n_r, n_x = g.shape
        values = np.empty((n_r * n_x, 3), dtype=np.float64)
        values[:, 0] = np.repeat(g[:, 0], n_x)
        values[:, 1] = np.tile(g[0, :], n_r)
        values[:, 2] = h.reshape(-1)
        return values

    @staticmethod
    def checkSingleCrossing(resultH) -> bool:
        return bool(check_table("single_crossing", resultH)[0])

    @staticmethod
    def checkNonIncreasing(arr) -> bool:
        return bool(check_table("non_increasing", arr)[0])

    @staticmethod
    def checkNonDecreasing(arr) -> bool:
        return bool(check_table("non_decreasing", arr)[0])
