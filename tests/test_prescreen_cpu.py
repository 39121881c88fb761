"""The prescreen without a device: the restatement and the constructed cases hold what they claim, the certificate verifier accepts the analytic
certificate and rejects broken ones, the new ABI entries validate their arguments, and the kernel's own per-control-point arithmetic (its
host twin, library-internal) meets the certificate contract on the constructed cases."""
import ctypes as C

import numpy as np
import pytest

from tests import feasibility as F
from tests import prescreen_cases as PC
from tests import prescreen_reference as PR

SHAPES = sorted(PC.SHAPES)


def _model(O, cs, case, rows=None):
    ag, lsc, sfc = F.oracle_inputs(O, case.inst.hdr, case.inst.rows if rows is None else rows, case.inst.sfc)
    return O.assemble(cs.oracle_class(O), ag, lsc, sfc)


def _analytic_cert(api, cs, case):
    """Uniform weights over the planted rows of a k-row case (their unit normals sum to zero): proven violation = s."""
    cp, k = case.cps[0], case.kind
    cert = np.zeros((), api.PRESCREEN_CERT_DTYPE)
    cert["fired"], cert["control_point"], cert["n_rows"] = 1, cp, k
    cert["row"][:k] = [j * cs.ci.P + cp for j in range(k)]
    cert["lambda"][:k] = 1.0 / k
    ids, N, b = PR.point_rows(cs.ci, case.inst.hdr, case.inst.rows, case.inst.sfc, cp)
    sel = [int(np.flatnonzero(ids == r)[0]) for r in cert["row"][:k]]
    rho, v = N[sel].mean(axis=0), b[sel].mean()
    p0 = np.asarray(case.inst.hdr["p0"], float)[:cs.ci.dim]
    D = np.sqrt((np.maximum(np.abs(cs.ci.world_min[:cs.ci.dim] - p0), np.abs(cs.ci.world_max[:cs.ci.dim] - p0)) ** 2).sum())
    cert["violation"] = v - np.abs(rho).sum() * D
    return cert


@pytest.mark.parametrize("shape", SHAPES)
def test_constructed_cases_are_what_they_claim(api, shape):
    cs = PC.build(api, shape)
    planted = [c for c in cs.cases if c.kind in (2, 3, 4, "face")]
    for c in planted:
        assert abs(c.t_planted - c.s) <= 1e-9, (c.kind, c.cps, c.s, c.t_planted)
    labels = [c.label for c in cs.cases]
    assert labels.count(PR.FIRE) >= 30 and labels.count(PR.QUIET) >= 30, (labels.count(PR.FIRE), labels.count(PR.QUIET))
    assert 3 * labels.count(PR.WINDOW) <= len(labels)
    # the places the construction exists for
    P = cs.ci.P
    assert {3, P - 1} <= {c.cps[0] for c in planted}
    if shape == "m12":
        assert any(c.cps[0] >= 64 for c in planted if c.label == PR.FIRE)
    assert any(c.kind == "two" for c in cs.cases) and any(c.kind == "fixed" for c in cs.cases)
    for c in cs.cases:
        if c.kind == "fixed":  # violated at the fixed point, and the QP's own rows untouched by it
            assert c.t_planted >= 1e-3 - 1e-9 and c.label == PR.QUIET


@pytest.mark.parametrize("shape", ["c1", "c0"])
def test_verifier_accepts_the_analytic_certificate_and_rejects_broken_ones(api, oracle, shape):
    cs = PC.build(api, shape)
    good = [c for c in cs.cases if c.kind in (2, 3, 4) and c.s >= 2e-5][:6]
    assert len(good) == 6
    for c in good:
        model = _model(oracle, cs, c)
        cert = _analytic_cert(api, cs, c)
        assert abs(PR.verify_cert(cs.ci, c.inst.hdr, c.inst.rows, model, cert) - c.s) <= 1e-9
        bad = cert.copy()
        bad["row"][0] += 1  # a row of the neighbouring control point
        with pytest.raises(PR.CertError):
            PR.verify_cert(cs.ci, c.inst.hdr, c.inst.rows, model, bad)
        bad = cert.copy()
        bad["row"][0] = -1 - 2 * cs.ci.dim  # a face of an axis the class does not have
        with pytest.raises(PR.CertError):
            PR.verify_cert(cs.ci, c.inst.hdr, c.inst.rows, model, bad)
        bad = cert.copy()
        bad["lambda"][0], bad["lambda"][1] = -0.25, bad["lambda"][1] + bad["lambda"][0] + 0.25
        with pytest.raises(PR.CertError):
            PR.verify_cert(cs.ci, c.inst.hdr, c.inst.rows, model, bad)
        bad = cert.copy()
        bad["violation"] += 1e-8  # not what the rows give
        with pytest.raises(PR.CertError):
            PR.verify_cert(cs.ci, c.inst.hdr, c.inst.rows, model, bad)
    for c in [c for c in cs.cases if c.kind in (2, 3, 4) and c.s < PR.PROOF_BAR][:4]:  # s below the bar: nothing to certify
        with pytest.raises(PR.CertError):
            PR.verify_cert(cs.ci, c.inst.hdr, c.inst.rows, _model(oracle, cs, c), _analytic_cert(api, cs, c))


def test_constants_are_the_headers(api):
    import os
    import re

    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lscqp.h")).read()
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, txt).group(1))  # noqa: E731
    assert api.INFO_PRESCREENED == val("LSCQP_INFO_PRESCREENED") == 128
    assert (api.PRESCREEN_OFF, api.PRESCREEN_ON) == (val("LSCQP_PRESCREEN_OFF"), val("LSCQP_PRESCREEN_ON"))
    assert api.PRESCREEN_CERT_DTYPE.itemsize == 72
    m = re.search(r"typedef struct lscqp_prescreen_cert \{(.*?)\} lscqp_prescreen_cert;", txt, re.S)
    fields = re.findall(r"(int32_t|double)\s+(\w+)(?:\[(\d+)\])?;", m.group(1))
    assert [f[1] for f in fields] == list(api.PRESCREEN_CERT_DTYPE.names)
    for sym in ("lscqp_prescreen_batch_device", "lscqp_set_prescreen", "lscqp_prescreen"):
        assert sym in api.EXPORTED_SYMBOLS and getattr(api.lib(), sym)


def test_entries_validate_and_need_a_device(api):
    import torch

    L = api.lib()
    sol = api.Solver(api.make_desc(M=5, dim=3))
    h = sol._h
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    assert sol.prescreen() == api.PRESCREEN_OFF
    assert L.lscqp_set_prescreen(None, 1) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_set_prescreen(h, 2) == api.ERR_INVALID_ARGUMENT and sol.prescreen() == api.PRESCREEN_OFF
    assert L.lscqp_prescreen(None) == -1
    assert L.lscqp_prescreen_batch_device(None, 1, 1, p, p, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_prescreen_batch_device(h, -1, 1, p, p, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_prescreen_batch_device(h, 1, -1, p, p, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_prescreen_batch_device(h, 0, 1, None, None, None, None, None, None) == api.OK  # an empty batch
    assert L.lscqp_prescreen_batch_device(h, 1, 1, None, p, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_prescreen_batch_device(h, 1, 1, p, None, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_prescreen_batch_device(h, 1, 1, p, p, p, None, p, None) == api.ERR_INVALID_ARGUMENT  # the class has corridors
    assert L.lscqp_prescreen_batch_device(h, 1, 1, p, p, p, p, None, None) == api.ERR_INVALID_ARGUMENT
    if not torch.cuda.is_available():
        assert L.lscqp_prescreen_batch_device(h, 1, 1, p, p, p, p, p, None) == api.ERR_NO_DEVICE
        sol.set_prescreen(api.PRESCREEN_ON)  # the mode is the handle's: set and read back without a device
        assert sol.prescreen() == api.PRESCREEN_ON
        sol.set_prescreen(api.PRESCREEN_OFF)
        assert sol.prescreen() == api.PRESCREEN_OFF


@pytest.mark.parametrize("fmt", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_twin_meets_the_contract_on_the_constructed_cases(api, oracle, shape, fmt):
    """The kernel's per-control-point arithmetic, run on the host: every certificate verifies, t* >= 1e-5 fires at the right control point,
    t* <= 0.9e-6 does not."""
    cs = PC.build(api, shape)
    sol = api.Solver(cs.desc(api, row_format=api.ROWS_F32 if fmt == "f32" else api.ROWS_F64))
    cert = sol.prescreen_twin(*PC.to_batch(api, cs.cases, cs.n_obs, cs.M))
    fired = 0
    for c, ct in zip(cs.cases, cert):
        rows = PC.rows_as_f32(c.inst.rows) if fmt == "f32" else c.inst.rows
        label = c.label
        if fmt == "f32" and c.kind != "fixed":  # the rounded rows have their own t*
            t = max(PR.t_star_cp(cs.ci, c.inst.hdr, rows, c.inst.sfc, cp) for cp in c.cps)
            label = PR.label_of(max(t, np.delete(cs.base_t, c.cps).max()))
        if ct["fired"]:
            fired += 1
            PR.verify_cert(cs.ci, c.inst.hdr, rows, _model(oracle, cs, c, rows), ct)
            assert label != PR.QUIET, (c.kind, c.s, c.cps)
            if label == PR.FIRE and all(np.atleast_1d(c.s) >= 2e-5):
                assert ct["control_point"] == c.expect_cp, (c.kind, c.s, ct["control_point"], c.expect_cp)
        else:
            assert label != PR.FIRE, (c.kind, c.s, c.cps)
            assert ct["control_point"] == -1 and ct["n_rows"] == 0 and ct["violation"] == 0.0
    assert fired >= 30
