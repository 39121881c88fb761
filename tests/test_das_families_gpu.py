"""The dual active-set phase ALONE on the designed instances of tests/das_cases.py, held to the oracle and to the numpy restatement of the
method (tests/das_reference.py) -- step by step, not only at the answer of the pair of kernels.

Every parity test of the default path passes whether the phase solved an instance or gave up on it: the interior-point kernel behind it
returns the same optimum.  Here nothing stands behind the phase (LSCQP_ACTIVE_SET_ONLY), the inputs were chosen on the CPU so that the
method stays well inside the budgets (tests/test_das_cases.py), and a hand-over is a failure:
  * every case comes back OPTIMAL with LSCQP_INFO_ACTIVE_SET at the polished oracle's optimum (x 1e-8 m, objective 1e-8 relative, KKT of the
    reference's row-for-row model 1e-8, reported residuals 1e-9, gap 0); the degenerate group alone may instead be handed over with
    WHY_PIVOT or WHY_NO_STEP, and then the default path must return the optimum at the interior-point bar;
  * lscqp_info.iterations is the restatement's step count wherever the restatement decided every selection and ratio test by more than
    1e-6 m -- a wrong decode, a wrong row id, a wrong rotation takes other steps even where it ends at the same point;
  * every form of the kernel returns the same bits: 64 / 128 / 256 threads, first look peeled or not, table copy and staged rows on or off,
    16-byte rows (the cases' rows are float32 values), the default handle, and -- through the device entry -- the fused launch;
  * the budget edges das_kmax and das_steps end the phase exactly where the restatement says."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

from tests import das_cases as DC
from tests import helpers as H
from tests.test_das_cases import CLEAR_MARGIN, restated

pytestmark = pytest.mark.gpu

X_TOL, OBJ_TOL, KKT_TOL, RES_TOL, X_TOL_INTERIOR_POINT = 1e-8, 1e-8, 1e-8, 1e-9, 1e-6
SHAPE_IDS = ["M%dd%d%s" % s for s in DC.SHAPES]
WHY = {1: "CAPACITY", 2: "EMPTY_INTERVAL", 3: "ROWS", 4: "STEPS", 5: "NO_STEP", 6: "PIVOT", 7: "VERIFICATION", 8: "MULTIPLIER"}


def _groups(oracle, shape):
    """the cases of one shape by class: {key: (spec, cases, (hdr, rows, off, sfc), n_obs_max)}"""
    from lsc_dr_planner_amd import api

    out = OrderedDict()
    for c in DC.cases(oracle, *shape):
        out.setdefault(c.key, []).append(c)
    for key, cs in out.items():
        spec = cs[0].spec
        cls = DC.oracle_class(oracle, spec)
        arrays = H.abi_batch(api, oracle, cls, [c.agent for c in cs], [c.lsc for c in cs], [c.sfc if c.sfc is not None else DC.wide_box(oracle, spec) for c in cs], spec["M"])
        assert len(cs) <= 256
        out[key] = (spec, cs, arrays, int(arrays[0]["n_obs"].max()))
    return out


def _why(info, q):
    return "handed over: LSCQP_DAS_WHY_%s after %d steps" % (WHY.get(int(info["res_dual"][q]), "?%g" % info["res_dual"][q]), int(info["gap"][q]))


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8)) for f in ("x", "obj", "status", "info"))


def _objective(oracle, c, x):
    A = oracle.assemble(DC.oracle_class(oracle, c.spec), c.agent, c.lsc, c.sfc if c.sfc is not None else DC.wide_box(oracle, c.spec))
    return DC.objective(A, x)


@pytest.mark.parametrize("shape", DC.SHAPES, ids=SHAPE_IDS)
def test_the_phase_alone_finishes_every_designed_case_in_the_restatements_steps(api, oracle, torch_cuda, shape):
    for key, (spec, cases, (hdr, rows, off, sfc), n_obs) in _groups(oracle, shape).items():
        only = api.Solver(DC.abi_desc(api, spec, active_set=api.ACTIVE_SET_ONLY))
        both = api.Solver(DC.abi_desc(api, spec))
        G = only.solve_host(hdr, rows, off, sfc)
        D = both.solve_host(hdr, rows, off, sfc)
        info = G["info"]
        worst = dict(dx=0.0, dobj=0.0, steps=0, held=0)
        agree = excluded = 0
        handed, wrong = [], []
        for q, c in enumerate(cases):
            r, g = c.oracle, restated(oracle, c)
            if G["status"][q] != 0:
                handed.append((c.name, _why(info, q)))
                ok = c.group == "degenerate" and G["status"][q] == api.STATUS_ITER_LIMIT and int(info["res_dual"][q]) in (api.DAS_WHY_PIVOT, api.DAS_WHY_NO_STEP)
                if ok:  # a truly dependent active set: the default path returns the optimum, by the interior-point kernel
                    ok = D["status"][q] == 0 and np.abs(D["x"][q] - r["x"]).max() <= X_TOL_INTERIOR_POINT
                if not ok:
                    wrong.append((c.name, "status %d" % G["status"][q], _why(info, q)))
                continue
            ref = _objective(oracle, c, r["x"])
            dx, dobj = np.abs(G["x"][q] - r["x"]).max(), abs(G["obj"][q] - ref) / max(1.0, abs(ref))
            worst["dx"], worst["dobj"] = max(worst["dx"], dx), max(worst["dobj"], dobj)
            worst["steps"], worst["held"] = max(worst["steps"], int(info["iterations"][q])), max(worst["held"], g["peak"])
            if not (info["flags"][q] & api.INFO_ACTIVE_SET):
                wrong.append((c.name, "no LSCQP_INFO_ACTIVE_SET"))
            if not (dx <= X_TOL and dobj <= OBJ_TOL):
                wrong.append((c.name, "dx %.2e dobj %.2e" % (dx, dobj)))
            if not (info["res_primal"][q] <= RES_TOL and info["res_dual"][q] <= RES_TOL and info["gap"][q] == 0):
                wrong.append((c.name, "residuals %.2e %.2e gap %g" % (info["res_primal"][q], info["res_dual"][q], info["gap"][q])))
            stat, eqv, iqv = H.kkt_from_primal(oracle, DC.oracle_class(oracle, spec), c.agent.reshape(1), c.lsc, c.sfc if c.sfc is not None else DC.wide_box(oracle, spec), G["x"][q])
            if not (stat <= KKT_TOL and eqv <= KKT_TOL and iqv <= KKT_TOL):
                wrong.append((c.name, "kkt %.2e %.2e %.2e" % (stat, eqv, iqv)))
            if g["margin"] > CLEAR_MARGIN:
                agree += 1
                if int(info["iterations"][q]) != g["steps"]:
                    wrong.append((c.name, "%d steps, the restatement takes %d (margin %.1e m at %s)" % (info["iterations"][q], g["steps"], g["margin"], g["margin_at"])))
            else:
                excluded += 1
            # what the phase finished, the default path returns bit for bit
            if not (D["status"][q] == 0 and np.array_equal(D["x"][q], G["x"][q]) and D["obj"][q] == G["obj"][q] and D["info"][q] == info[q]):
                wrong.append((c.name, "the default handle differs from the phase alone"))
        fams = sorted({c.expect["family"] for c in cases if c.expect and c.expect["family"]} | {"leaving" for c in cases if c.name.startswith("leaving")})
        print("r11| M%d d%d %-4s | %3d cases | %s | steps <= %d, rows held <= %d | max |dx| %.1e m, objective %.1e rel | steps agree on %d, %d below the margin | handed over: %s"
              % (key + (len(cases), ",".join(fams), worst["steps"], worst["held"], worst["dx"], worst["dobj"], agree - sum("steps, the" in w[1] for w in wrong), excluded, handed or "none")))
        assert not wrong, wrong
        assert agree > 0 or len(cases) == 1


@pytest.mark.parametrize("shape", DC.SHAPES, ids=SHAPE_IDS)
def test_every_form_of_the_kernel_returns_the_same_bits(api, oracle, torch_cuda, shape):
    for key, (spec, cases, (hdr, rows, off, sfc), n_obs) in _groups(oracle, shape).items():
        base = api.Solver(DC.abi_desc(api, spec, active_set=api.ACTIVE_SET_ONLY)).solve_host(hdr, rows, off, sfc)
        assert base["info"]["iterations"].max() >= 1 or len(cases) == 1
        for threads in (64, 128, 256):
            for loop in (0, 1):
                for cache in (0, 1):
                    for stage in (0, 1):
                        sol = api.Solver(DC.abi_desc(api, spec, active_set=api.ACTIVE_SET_ONLY))
                        for k, v in (("das_threads", threads), ("das_loop", loop), ("das_cache", cache), ("das_stage", stage)):
                            sol.set_knob(k, v)
                        assert _same(sol.solve_host(hdr, rows, off, sfc), base), (key, threads, loop, cache, stage)
        # 16-byte rows: every row of the cases is a float32 value
        assert np.array_equal(rows["b"], np.float32(rows["b"])) and np.array_equal(rows["nx"], np.float32(rows["nx"]))
        f32 = api.Solver(DC.abi_desc(api, spec, active_set=api.ACTIVE_SET_ONLY, row_format=api.ROWS_F32))
        assert _same(f32.solve_host(hdr, rows, off, sfc), base), key
        for threads in (64, 128):
            f32.set_knob("das_threads", threads)
            assert _same(f32.solve_host(hdr, rows, off, sfc), base), (key, threads)


@pytest.mark.parametrize("shape", DC.FUSED_SHAPES, ids=["M%dd%d%s" % s for s in DC.FUSED_SHAPES])
def test_the_fused_launch_returns_the_phases_bits_on_the_designed_cases(api, oracle, torch_cuda, shape):
    from tests.test_das_fused import _Dev, _kernel_nodes

    torch = torch_cuda
    key = shape
    spec, cases, arrays, n_obs = _groups(oracle, shape)[key]
    n = len(cases)
    assert n <= torch.cuda.get_device_properties(0).multi_processor_count  # (one instance per CU at most: the fused launch's condition)
    alone = api.Solver(DC.abi_desc(api, spec, active_set=api.ACTIVE_SET_ONLY)).solve_host(*arrays)
    by_phase = alone["status"] == 0  # (everything but, possibly, the degenerate group: the first test of this module)
    assert all(by_phase[q] for q, c in enumerate(cases) if c.group == "main")
    res = {}
    for fused in (1, 0):
        sol = api.Solver(DC.abi_desc(api, spec))
        sol.set_knob("das_fused", fused)
        if shape == (10, 3, "lsc"):
            # The fused form of this shape is carved for 20 active rows (lscqp_fused.hip, FusedCarve: its staged rows leave no room for 32) and
            # refuses the 32 the policy gives a batch of few obstacles -- which then runs the two launches.  With the budget the configs[3] shard
            # gets, the fused kernel runs; the cases hold at most 9 rows, and the phase alone above keeps the policy's 32.
            sol.set_knob("das_kmax", 20)
        d = _Dev(torch, sol, n, n_obs, arrays, None)
        d.solve()
        x, obj, st, info = d.result()
        res[fused] = dict(x=x.reshape(n, -1), obj=obj, status=st, info=info.view(api.INFO_DTYPE))
        d.clear()
        assert _kernel_nodes(torch, d) == (1 if fused else 2), fused  # (the fused form did run / did not)
    assert _same(res[1], res[0])
    assert (res[1]["status"] == 0).all() and ((res[1]["info"]["flags"][by_phase] & api.INFO_ACTIVE_SET) != 0).all()
    assert _same({f: v[by_phase] for f, v in res[1].items()}, {f: v[by_phase] for f, v in alone.items()})


def _lds_bytes(api, M, dim, kmax, cache, stage_rows):
    L = api.lib()
    L.lscqp_das_lds_bytes.restype = C.c_size_t
    L.lscqp_das_lds_bytes.argtypes = [C.c_int] * 5
    return L.lscqp_das_lds_bytes(M, dim, kmax, cache, stage_rows)


@pytest.mark.parametrize("shape", [(5, 3, "lsc"), (10, 3, "lsc"), (6, 3, "dlsc")], ids=["M5d3lsc", "M10d3lsc", "M6d3dlsc"])
def test_the_budget_edges_end_the_phase_where_the_restatement_says(api, oracle, torch_cuda, shape):
    spec, cases, _, _ = _groups(oracle, shape)[shape]
    # the case with the most steps among those that decide every step clearly, hold at least three rows and drop one
    pick = [c for c in cases if c.group == "main" and restated(oracle, c)["margin"] > CLEAR_MARGIN and restated(oracle, c)["peak"] >= 3 and restated(oracle, c)["left"]]
    assert pick, "no case with a leaving row and a clear margin on this shape"
    c = max(pick, key=lambda c: restated(oracle, c)["steps"])
    g = restated(oracle, c)
    M, dim = spec["M"], spec["dim"]
    hdr, rows, off, sfc = H.abi_batch(api, oracle, DC.oracle_class(oracle, spec), [c.agent], [c.lsc], [c.sfc if c.sfc is not None else DC.wide_box(oracle, spec)], M)
    n_obs = int(hdr["n_obs"].max())
    # the launch policy lowers no knob set here: the footprint with the table copy and the staged rows fits the CU's LDS
    assert _lds_bytes(api, M, dim, 32, 1, n_obs * 6 * M) <= 160 * 1024

    def run(knob, value, active_set):
        sol = api.Solver(DC.abi_desc(api, spec, active_set=active_set))
        sol.set_knob(knob, value)
        return sol.solve_host(hdr, rows if c.lsc is not None else None, off if c.lsc is not None else None, sfc)

    for knob, enough, why in (("das_kmax", g["peak"], api.DAS_WHY_ROWS), ("das_steps", g["steps"], api.DAS_WHY_STEPS)):
        G = run(knob, enough, api.ACTIVE_SET_ONLY)
        assert G["status"][0] == 0 and G["info"]["iterations"][0] == g["steps"], (c, knob, enough, G["status"], _why(G["info"], 0))
        assert np.abs(G["x"][0] - c.oracle["x"]).max() <= X_TOL
        G = run(knob, enough - 1, api.ACTIVE_SET_ONLY)
        assert G["status"][0] == api.STATUS_ITER_LIMIT and int(G["info"]["res_dual"][0]) == why, (c, knob, enough - 1, G["status"], _why(G["info"], 0))
        D = run(knob, enough - 1, api.ACTIVE_SET_DEFAULT)  # the default path: the interior-point kernel's answer
        assert D["status"][0] == 0 and not (D["info"]["flags"][0] & api.INFO_ACTIVE_SET)
        assert np.abs(D["x"][0] - c.oracle["x"]).max() <= X_TOL_INTERIOR_POINT
