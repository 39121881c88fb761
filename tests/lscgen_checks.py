"""What the LSC generator tests hold a run to (tests/test_lscgen.py, tests/test_lscmode.py) -- TEST INFRASTRUCTURE.

Standing bars of this kernel: 2e-7 on a normal component, 2e-6 on b (4e-6 under LSCQP_ROWS_F32); exactness claims are ==."""
import numpy as np

from tests import lscgen_cases as LC

TOL_N, TOL_B, TOL_B_F32 = 2e-7, 2e-6, 4e-6
# Device against the referee where no constructed answer exists (golden hulls, slivers): the error is the float32 cast of the closest
# point, the float32 norm and division, and the conditioning of small distances -- measured, not derived.  ORACLE_DEV is the oracle's
# worst deviation from the referee on the CPU, per family (normal component, b), as test_oracle_against_referee_* measure and assert it;
# the device bar is that plus one float32 ulp of the value (the device may round one sqrtf or one division the other way).
ORACLE_DEV = {"sliver": (2.0e-8, 4.8e-8), "golden3d": (1.2e-7, 7.9e-7), "golden2d": (1.13e-7, 5.6e-7)}  # measured: 1.99e-8, 4.72e-8; 1.199e-7, 7.86e-7; 1.129e-7, 5.57e-7


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _dev(got, want):
    """largest |got - want| over normal components and over b, where want is stated (not NaN)"""
    m = ~np.isnan(want)
    assert m.any()
    d = np.abs(np.where(m, got - want, 0.0))
    return d[..., :3].max(), d[..., 3].max()


def _hold(got, want, tol_n=TOL_N, tol_b=TOL_B, what=""):
    dn, db = _dev(got, want)
    print("%s: normal %.3g  b %.3g" % (what, dn, db))
    assert np.isfinite(got).all(), what
    assert dn <= tol_n and db <= tol_b, (what, dn, db)


def _hold_to_referee(got, want, family, what=""):
    """device against the referee at ORACLE_DEV[family] + one float32 ulp of each value"""
    m = ~np.isnan(want)
    d = np.abs(np.where(m, got - want, 0.0))
    bar = np.where(m, _ulp32(np.where(m, want, 0.0)), 0.0)
    bar[..., :3] += ORACLE_DEV[family][0]
    bar[..., 3] += ORACLE_DEV[family][1]
    print("%s: normal %.3g  b %.3g  (bars %.3g + ulp, %.3g + ulp)" % (what, d[..., :3].max(), d[..., 3].max(), *ORACLE_DEV[family]))
    assert (d <= bar).all(), (what, d[..., :3].max(), d[..., 3].max())


def _family_mask(cases, pk, families, keep=True):
    """(N, M) mask of the units whose case is (keep) / is not (not keep) in `families`"""
    s = pk["slot"]
    fam = np.array([c["family"] in families for c in cases] + [False])
    return (s >= 0) & (fam[s] == keep)


def _masked(want, mask):
    w = want.copy()
    w[~mask] = np.nan
    return w


def _exact_claims(cases, pk, got, mode):
    """what holds with ==: nz and the z term of b in 2-D; generateCLSC on a hull around the origin: zero normal, b = (r_a + r_b) / 2"""
    N, M = pk["N"], pk["M"]
    if pk["dim"] == 2:
        assert (got[..., 2] == 0).all()
    for a in range(N):
        for m in range(M):
            ci = pk["slot"][a, m]
            if ci < 0:
                continue
            zero = cases[ci]["kind"] == "inside" and (mode == "clsc" or cases[ci]["fb"] == "zero")
            if zero and "radius" in pk and "nbr" in pk:
                assert (got[a, m, :, :3] == 0).all() and (got[a, m, :, 3] == 0.5 * (pk["radius"][a] + pk["radius"][N + a])).all(), cases[ci]["name"]
            elif zero:
                assert (got[a, m, :, :3] == 0).all() and (got[a, m, :, 3] == pk["table"][a]["radius"] + pk["radius"][a]).all(), cases[ci]["name"]


def _coverage_line(cases, pk, dim, what):
    won = {cases[ci]["winner"] for ci in pk["slot"].ravel() if ci >= 0 and cases[ci]["family"].startswith("feature")}
    feats = LC.FEATURES_3D if dim == 3 else LC.FEATURES_2D
    print("coverage %s: %d of %d hull features won on the device in %d-D" % (what, len(won & set(feats)), len(feats), dim))
    assert won >= set(feats)


def _hold_device(cases, pk, got, oracle_rows, n_con, n_ref, mode, expected, rows_f32=False):
    """the three holds of one device run: constructed result, referee, oracle"""
    tol_b = TOL_B_F32 if rows_f32 else TOL_B
    sliver = _family_mask(cases, pk, ("sliver",))
    rest = _family_mask(cases, pk, ("sliver",), keep=False)
    _hold(got, _masked(expected(n_con), rest), TOL_N, tol_b, what="device %s vs constructed" % mode)
    _hold(got, _masked(expected(n_ref), rest), TOL_N, tol_b, what="device %s vs referee" % mode)
    if sliver.any():
        if rows_f32:  # (b is rounded to float32 on the way out: the format's standing bar)
            _hold(got, _masked(expected(n_ref), sliver), ORACLE_DEV["sliver"][0] + 2.0 ** -24, tol_b, what="device %s slivers vs referee" % mode)
        else:
            _hold_to_referee(got, _masked(expected(n_ref), sliver), "sliver", what="device %s slivers vs referee" % mode)
    _hold(got, oracle_rows, TOL_N, tol_b, what="device %s vs oracle" % mode)
    _exact_claims(cases, pk, got, mode)
