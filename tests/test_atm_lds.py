"""The coarse ISA atmosphere table and the wind slopes that the 512-thread step kernels hold in LDS
(DESIGN.md s5, s8), checked on the host, no GPU.

pd_atm_table_lds builds the coarse table as pd_create does and evaluates it in the device's order;
it must equal the oracle's closed form (oracle/pd_oracle.c orc_atmosphere) at the bounds
tests/test_atm_table.py sets for the fine table: <= 1e-14 relative, median <= 1e-15 -- at 1e5
altitudes, at every layer boundary +- 2 m (the table takes the closed form's side of the pb jump)
and at every cell edge.  pd_wind_slopes returns the tabulated slopes of the wind profiles'
intervals: the bits of np_interp's division on the same operands."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib_params():
    from pdenv import _lib, params
    return _lib.load(), params.Params()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _table(L, P, alt):
    alt = np.ascontiguousarray(alt, dtype=np.float64)
    atm, err, nc = np.zeros((len(alt), 3)), np.zeros(1), C.c_int32(0)
    assert L.pd_atm_table_lds(C.byref(P.struct), _ptr(alt), len(alt), _ptr(atm), _ptr(err), C.byref(nc)) == 0
    return atm, float(err[0]), nc.value


def _boundaries(P):
    r = P.struct.isa_r
    hb = np.array(P.struct.isa_Hb[:])
    yb = r * hb[hb > 0] / (r - hb[hb > 0])
    return yb[yb < P.struct.isa_alt_max]


def _oracle(alt):
    import oracle
    ol, op = oracle.lib(), C.byref(oracle.params())
    ref = np.zeros((len(alt), 3))
    r, p, a = C.c_double(), C.c_double(), C.c_double()
    for i, y in enumerate(alt):
        ol.orc_atmosphere(op, float(y), C.byref(r), C.byref(p), C.byref(a))
        ref[i] = (r.value, p.value, a.value)
    return ref


def test_coarse_table_against_the_oracle(lib_params):
    L, P = lib_params
    top = P.struct.isa_alt_max
    _, err, n_cells = _table(L, P, np.zeros(1))
    assert err <= 1e-14, err            # the builder's check against the long double closed form
    w = 1000.0                          # the cell width (pd_physics.h kAtlW)
    assert n_cells == int(np.ceil(top / w))
    rng = np.random.default_rng(5)
    edges = np.arange(1, n_cells) * w
    pts = [np.linspace(0.0, top * (1 - 1e-12), 50000), rng.uniform(0, top, 50000),
           (_boundaries(P)[:, None] + np.linspace(-2.0, 2.0, 81)[None, :]).ravel(),
           np.concatenate([np.nextafter(edges, 0.0), edges, np.nextafter(edges, np.inf), edges - 1e-6, edges + 1e-6])]
    alt = np.concatenate(pts)
    alt = alt[(alt >= 0) & (alt < top)]
    assert len(alt) >= 100000
    atm, _, _ = _table(L, P, alt)
    ref = _oracle(alt)
    rel = np.abs(atm - ref) / np.abs(ref)
    print("coarse table: max rel", rel.max(0), "median", np.median(rel))
    assert rel.max() <= 1e-14, (rel.max(0), alt[rel.max(1).argmax()])
    assert np.median(rel) <= 1e-15
    # outside the ISA's range, and below the ground (clamped to 0), as the closed form
    out, _, _ = _table(L, P, np.array([top, top + 1.0, -5.0, 0.0]))
    assert (out[:2] == 0).all() and np.array_equal(out[2], out[3])


def test_wind_slopes_are_np_interp_division(lib_params):
    L, P = lib_params
    s = P.struct
    got = np.zeros((50, 16))
    assert L.pd_wind_slopes(C.byref(s), _ptr(got)) == 0
    x = np.array([list(r) for r in s.wind_alt_km], dtype=np.float64)
    y = np.array([list(r) for r in s.wind_speed], dtype=np.float64)
    n = np.array(s.wind_n[:])
    want = np.zeros((50, 16))
    for w in range(50):
        for j in range(int(n[w]) - 1):
            # numpy compiled_base.c arr_interp: slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
            want[w, j] = (y[w, j + 1] - y[w, j]) / (x[w, j + 1] - x[w, j])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
