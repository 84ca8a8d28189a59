"""Mixed quadrilateral / triangle meshes on the device, against the genuine reference's fixtures under tests/golden/mixed2d
(tools/capture_mixed2d.py; tests/test_mixed2d_oracle.py shows without a GPU that every input here is a sound one): the per-method
path (fused 0) and, with option blocks_2d 1, the 2-D simplex fused stage over several two-dimensional blocks (csrc/simplex2d.hip;
hfx_run_steps_blocks(..., fused = 4)): one element and one update launch per block, the interior-face blocks between two element
blocks (cross blocks) with each side's arrays from its own block, quadrilaterals on the dense kernels' second size table.

Bars, relative to the array's largest magnitude: 1e-12 for one residual's intermediates, 5e-11 for div_tconf_upts, 1e-11 for states
after whole steps, 1e-12 for disu_fpts against opp_0 of the new state.  Every fused run asserts hfx_simplex2d_stage_plan and every
block's hfx_simplex2d_plan against the size tables, so a silent per-method run cannot pass.  Blocks of G - 1, G + 1 and 2 G + 1
elements of EACH class's own G come from tests/mixed2d_util.py and are checked against the oracle on the same block.

Without the block stage every fused test here fails: option blocks_2d is unknown and the calls are refused.  The per-method tests pass."""
import numpy as np
import pytest

import hfx
import mixed2d_util as X
import mixed_util as MU
import tri_util as T
from test_gpu_methods_vs_golden import build

pytestmark = pytest.mark.gpu

TOL_1, TOL_DIV, TOL_U, TOL_FPTS = 1e-12, 5e-11, 1e-11, 1e-12
FIXTURES = ["mx_p1_n4", "mx_p2_n4", "mx_p3_n4", "mx_p4_n4", "mx_p3_walls", "mx_p2_inviscid", "mx_p2_roem_sutherland", "mx_p2_rusanov_ldg"]
relerr = T.relerr
GPU_ARRAYS = {"s0_disu_fpts": "DISU_FPTS", "s0_tdisf_upts": "TDISF_UPTS", "s0_norm_tdisf_fpts": "NORM_TDISF_FPTS",
              "s0_delta_disu_fpts": "DELTA_DISU_FPTS", "s0_grad_disu_upts": "GRAD_DISU_UPTS", "s0_grad_disu_fpts": "GRAD_DISU_FPTS",
              "s0_div_tconf_upts": "DIV_TCONF_UPTS"}


@pytest.fixture()
def ctx():
    c = hfx.Context(0)
    c.set_option("blocks_2d", 1)
    yield c
    c.close()


def make(ctx, d):
    """-> (classes, {class: Eles}, face blocks, [(left class, right class)] of the interior ones, boundary blocks)"""
    classes, per, faces, bdy = MU.split(d)
    ctx.set_params(hfx.params_from(per[classes[0]]))
    ctx.set_contract_mode(hfx.CONTRACT_AUTO)
    E = {}
    for c in classes:
        sz = [int(v) for v in per[c]["sizes"]]
        E[c] = hfx.Eles(ctx, sz[:5], per[c], ele_type=sz[6], order=sz[5])
        E[c].upload(hfx.DISU_UPTS0, per[c]["u_init"])
    F = [hfx.IntInters(ctx, E[a], E[b], L, R) for a, b, L, R in faces]
    B = [hfx.BdyInters(ctx, E[a], L, ids, hfx.bc_records(d["bc_flags"], d["bc_params"]), float(np.ravel(d["bc_R_ref"])[0]),
                       int(np.ravel(d["ramp_counter"])[0])) for a, L, ids in bdy]
    return classes, E, F + B, [(a, b) for a, b, _, _ in faces], B


def close(E, F):
    for f in F:
        f.close()
    for e in E.values():
        e.close()


def viscous(d):
    return bool(int(np.ravel(d["viscous"])[0]))


def expected_plan(d, c, pairs, gather=1):
    """hfx_simplex2d_plan of class c's block (label c; the element class is in its sizes), from the size tables"""
    sz = [int(v) for v in d["c%d_sizes" % c]]
    nu, nfp, order, cls = sz[1], sz[2], sz[5], sz[6]
    assert (nu, nfp) == X.POINTS[cls][order]
    g = X.GROUP[cls][order]
    inside = (c, c) in pairs
    plan = {"size_class": X.SIZE_CLASS[cls](order), "group": g, "waves": 4, "gather": int(bool(gather) and viscous(d) and inside),
            "element_lds": 8 * (4 * nu * nu + 6 * nu * nfp + (g + 1) * (12 * nu + 4 * nfp)),
            "update_lds": 8 * (2 * nu * nfp + (g + 1) * (4 * nu + 4 * nfp))}
    assert plan["element_lds"] <= X.LDS_BUDGET and nu * g <= 512
    return plan


def expected_stage_plan(d, classes, pairs, n_bdy, gather=1):
    cross = sum(a != b for a, b in pairs)
    delta = (cross + (0 if gather else len(pairs) - cross)) if viscous(d) else 0
    return {"blocks": len(classes), "interior_face_blocks": len(pairs), "cross_face_blocks": cross, "delta_launches": delta,
            "launches": (2 if viscous(d) else 1) * n_bdy + delta + 2 * len(classes) + len(pairs)}


def check_fpts_and_nan(d, classes, E, what):
    for c in classes:
        u = E[c].download(hfx.DISU_UPTS0)
        err = relerr(E[c].download(hfx.DISU_FPTS), np.einsum("fu,uen->fen", np.asarray(d["c%d_opp_0" % c] if "c%d_opp_0" % c in d else d["opp_0"]), u))
        print("%s class %d: disu_fpts against opp_0 u %.2e" % (what, c, err))
        assert err < TOL_FPTS, (what, c, err)
        assert E[c].check_nan() == -1, (what, c)


def final_states(d):
    """[{class: state after the step} or None] per step of a fixture"""
    classes = X.classes_of(d)
    nstage = X.sizes(d, classes[0])[7]
    out = []
    for st in range(max(X.stored_steps(d)) + 1):
        k = "u_step%d_stage%d" % (st, nstage - 1)
        out.append({c: {"u": d["c%d_%s" % (c, k)]} for c in classes} if "c%d_%s" % (classes[0], k) in d else None)
    return out


# ---- 1. the per-method path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_per_method_states(name):
    """hfx_CalcResidual_blocks + AdvanceSolution per block: every dumped stage state of both classes, and on mx_p2_n4 what one
    residual leaves in the public arrays"""
    d = X.load(name)
    c0 = hfx.Context(0)
    classes, E, F, pairs, B = make(c0, d)
    blocks = [E[c] for c in classes]
    nstage, adv = X.sizes(d, classes[0])[7], int(np.ravel(d["adv_type"])[0])
    for st in range(max(X.stored_steps(d)) + 1):
        for rk in range(nstage):
            hfx.CalcResidual_blocks(blocks, F)
            if st == 0 and rk == 0:
                for key, arr in GPU_ARRAYS.items():
                    for c in classes:
                        k = "c%d_%s" % (c, key)
                        if k in d and (viscous(d) or "grad" not in key and "delta" not in key):
                            err, bar = relerr(E[c].download(getattr(hfx, arr)), d[k]), TOL_DIV if "div" in key else TOL_1
                            print("%-28s %.2e" % (k, err))
                            assert err < bar, (k, err)
            for c in classes:
                E[c].AdvanceSolution(rk, adv)
            for c in classes:
                k = "c%d_u_step%d_stage%d" % (c, st, rk)
                if k in d:
                    assert relerr(E[c].download(hfx.DISU_UPTS0), d[k]) < TOL_U, k
    for c in classes:
        assert E[c].check_nan() == -1
    close(E, F)
    c0.close()


@pytest.mark.parametrize("name", ["mx_p3_n4", "mx_p3_walls"])
def test_per_method_loop(name):
    d = X.load(name)
    c0 = hfx.Context(0)
    classes, E, F, pairs, B = make(c0, d)
    for st, w in enumerate(final_states(d)):
        hfx.run_steps_blocks([E[c] for c in classes], F, 1, fused=0)
        for c in classes:
            assert relerr(E[c].download(hfx.DISU_UPTS0), w[c]["u"]) < TOL_U, (st, c)
    close(E, F)
    c0.close()


# ---- 2. the block stage ----------------------------------------------------------------------------------------------------------
def run_fused(ctx, d, want, what, gather=1, steps_per_call=1, opts=()):
    """fused 4 with option blocks_2d 1 over the blocks of d; want: per step {class: {"u": ..}} or None -> ({class: final state},
    stage plan)"""
    ctx.set_option("gather_delta", gather)
    for k, v in opts:
        ctx.set_option(k, v)
    classes, E, F, pairs, B = make(ctx, d)
    blocks = [E[c] for c in classes]
    st = 0
    while st < len(want):
        hfx.run_steps_blocks(blocks, F, steps_per_call, fused=4)
        st += steps_per_call
        w = want[st - 1]
        if w is not None:
            for c in classes:
                u = E[c].download(hfx.DISU_UPTS0)
                per_ele = np.abs(u - w[c]["u"]).max(axis=(0, 2)) / np.abs(w[c]["u"]).max()
                print("%s step %d class %d: state %.2e (element %d of %d)" % (what, st - 1, c, per_ele.max(), int(per_ele.argmax()), len(per_ele)))
                assert per_ele.max() < TOL_U, (what, st - 1, c, int(per_ele.argmax()), per_ele.max())
                if w[c].get("div") is not None:
                    err = relerr(E[c].download(hfx.DIV_TCONF_UPTS), w[c]["div"])
                    assert err < 10 * TOL_DIV, (what, st - 1, c, err)  # (of the step's LAST stage: the bar of tests/test_gpu_general_batches.py)
        check_fpts_and_nan(d, classes, E, "%s step %d" % (what, st - 1))
    sp = hfx.simplex2d_stage_plan(blocks)
    assert sp == expected_stage_plan(d, classes, pairs, len(B), gather), (sp, expected_stage_plan(d, classes, pairs, len(B), gather))
    for c in classes:
        assert E[c].simplex2d_plan() == expected_plan(d, c, pairs, gather), (c, E[c].simplex2d_plan())
    out = {c: E[c].download(hfx.DISU_UPTS0) for c in classes}
    ms, names = hfx.time_general_kernels(blocks, F, reps=1)  # (advances the state by a stage: behind the download)
    assert names.startswith("face_delta_kernel,simplex2d_element_kernel,face_flux2_kernel,simplex2d_update_kernel"), names
    by = hfx.general_kernel_bytes(blocks)
    assert by[1] > 0 and by[3] > 0 and (by[0] > 0) == (sp["delta_launches"] > 0)
    close(E, F)
    return out, sp


@pytest.mark.parametrize("gather", [1, 0])
@pytest.mark.parametrize("name", FIXTURES)
def test_fused_states(ctx, name, gather):
    """every fixture, the run cut into single-step calls: the state of both classes after every stored step, the NaN flag, the
    stage plan and both blocks' plans; the LDG corrections inside a block gathered by its element kernel (the default) or all of
    them written by face_delta_kernel<2>"""
    d = X.load(name)
    want = final_states(d)
    assert want[-1] is not None
    out, sp = run_fused(ctx, d, want, name, gather)
    assert sp["cross_face_blocks"] >= 1 and sp["blocks"] == 2


@pytest.mark.parametrize("name", ["mx_p1_n4", "mx_p3_n4"])
def test_fused_whole_run_in_one_call(ctx, name):
    """both steps in one call equal the genuine reference too (the other tests cut the run into single-step calls)"""
    d = X.load(name)
    want = final_states(d)
    run_fused(ctx, d, [None] * (len(want) - 1) + [want[-1]], name, steps_per_call=len(want))


@pytest.mark.parametrize("name", FIXTURES)
def test_deferred_call_sequence(name):
    """the reference's calls over both blocks with `deferred` 1: every whole stage runs as the block stage (n_fused; the plan query
    answers) and EVERY dumped stage state of both classes is met"""
    from test_gpu_deferred import calc_residual_calls, tag
    d = X.load(name)
    c1 = hfx.Context(0)
    c1.set_option("blocks_2d", 1)
    c1.set_option("deferred", 1)
    classes, E, F, pairs, B = make(c1, d)
    blocks = [E[c] for c in classes]
    for e in blocks:
        tag(e, d)
    nstage, adv = X.sizes(d, classes[0])[7], int(np.ravel(d["adv_type"])[0])
    n = 0
    for st in range(max(X.stored_steps(d)) + 1):
        for rk in range(nstage):
            calc_residual_calls(blocks, F, viscous(d), rk)
            for e in blocks:
                e.AdvanceSolution(rk, adv)
            n += 1
            for c in classes:
                k = "c%d_u_step%d_stage%d" % (c, st, rk)
                if k in d:
                    err = relerr(E[c].download(hfx.DISU_UPTS0), d[k])
                    assert err < TOL_U, (k, err)
    nf, nr, why = c1.deferred_stats()
    print("deferred: %d fused, %d replayed (%s)" % (nf, nr, why))
    assert (nf, nr) == (n, 0), (nf, nr, why)
    assert hfx.simplex2d_stage_plan(blocks) == expected_stage_plan(d, classes, pairs, len(B))
    for c in classes:
        assert E[c].simplex2d_plan() == expected_plan(d, c, pairs)
        assert E[c].check_nan() == -1
    close(E, F)
    c1.close()


# ---- 3. group edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_fused_group_edges(ctx, order, which):
    """per class G - 1, G + 1 and 2 G + 1 elements of that class's own G, both classes at once, cut out of the tiled fixture (every
    copy its own state), against the oracle on the same block; and element a + G is not taken for element a"""
    want = X.edge_counts(order)[which]
    d = X.block(order, want[X.TRI], want[X.QUAD])
    ref = X.reference(("block", order, want[X.TRI], want[X.QUAD]), d)
    assert all(r["bad"] == -1 for r in ref)
    out, sp = run_fused(ctx, d, ref, "P%d block of %d + %d" % (order, want[X.TRI], want[X.QUAD]))
    assert sp["cross_face_blocks"] >= 1
    for c in (X.TRI, X.QUAD):
        g = X.GROUP[c][order]
        if want[c] > g:
            diff = T.offset_differences(ref[-1][c]["u"], g)
            assert diff.min() > 100 * TOL_U, (c, diff.min())  # (the reference tells a + G from a: the state bar would see the slip)
            assert T.offset_differences(out[c], g).min() > 100 * TOL_U


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_quadrilateral_block_alone(ctx, order):
    """one block of 2 G + 1 quadrilaterals, fused 4 with the option on: the dense stage on the second size table"""
    g = X.GROUP[X.QUAD][order]
    d = X.quad_block(order, 2 * g + 1)
    ref = X.reference(("quad", order), d)
    e, faces = build(ctx, d)
    for st, w in enumerate(ref):
        hfx.run_steps_blocks([e], faces, 1, fused=4)
        err = relerr(e.download(hfx.DISU_UPTS0), w["u"])
        print("P%d quadrilaterals step %d: %.2e" % (order, st, err))
        assert err < TOL_U, (order, st, err)
        assert relerr(e.download(hfx.DISU_FPTS), np.einsum("fu,uen->fen", np.asarray(d["opp_0"]), e.download(hfx.DISU_UPTS0))) < TOL_FPTS
        assert e.check_nan() == -1
    nu, nfp = X.POINTS[X.QUAD][order]
    plan = e.simplex2d_plan()
    assert (plan["size_class"], plan["group"], plan["gather"]) == (5 + order - 1, g, 1), plan
    assert plan["element_lds"] == 8 * (4 * nu * nu + 6 * nu * nfp + (g + 1) * (12 * nu + 4 * nfp)) <= X.LDS_BUDGET
    sp = hfx.simplex2d_stage_plan([e])
    assert (sp["blocks"], sp["cross_face_blocks"], sp["delta_launches"]) == (1, 0, 0), sp
    for f in faces:
        f.close()
    e.close()


def test_several_triangle_blocks(ctx):
    """tri_p3_n4_deformed split into two element blocks with cross faces between them: the genuine reference's states, permuted"""
    d = T.load("tri_p3_n4_deformed")
    first = np.arange(int(d["sizes"][0])) % 3 != 0
    m = X.split_triangles(d, first)
    nstage = int(d["sizes"][7])
    want = [{0: {"u": d["u_step%d_stage%d" % (st, nstage - 1)][:, first]}, 2: {"u": d["u_step%d_stage%d" % (st, nstage - 1)][:, ~first]}} for st in range(2)]
    out, sp = run_fused(ctx, m, want, "two triangle blocks")
    assert sp["cross_face_blocks"] == 2 and sp["blocks"] == 2


def test_single_triangle_block_is_unchanged():
    """one triangle block with the option on: bit-equal to the option off, plan and all"""
    d = T.load("tri_p3_bdy")
    got = {}
    for on in (0, 1):
        c = hfx.Context(0)
        c.set_option("blocks_2d", on)
        e, faces = build(c, d)
        hfx.run_steps_blocks([e], faces, 2, fused=4)
        got[on] = (e.download(hfx.DISU_UPTS0), e.download(hfx.DIV_TCONF_UPTS), e.simplex2d_plan())
        for f in faces:
            f.close()
        e.close()
        c.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and got[0][2] == got[1][2]


# ---- 4. the per-step duties ------------------------------------------------------------------------------------------------------
def test_duties_in_the_fused_loop():
    """mx_p3_walls with the clock set: time averages and the residual history rows of both blocks in a fused-4 loop equal those of
    the fused-0 loop at 1e-12 per field / 1e-11 on the norm, as tests/test_gpu_tris.py does for triangles"""
    d = X.load("mx_p3_walls")
    fields = ["rho_average", "u_average", "v_average", "e_average"]
    out = {}
    for fused in (0, 4):
        c = hfx.Context(0)
        c.set_option("blocks_2d", 1)
        classes, E, F, pairs, B = make(c, d)
        for e in E.values():
            e.set_average_fields(fields)
        c.set_history_monitor(2, False, 1, capacity=4)
        c.set_clock(0.25, 0)
        hfx.run_steps_blocks([E[k] for k in classes], F, 3, fused=fused)
        out[fused] = {}
        for k in classes:
            times, steps, res, frc = E[k].read_history()  # (empties the block's history: once)
            out[fused][k] = (E[k].download_average(), np.array(steps), np.array(res))
        out[fused]["clock"] = c.get_clock()
        if fused == 4:
            assert hfx.simplex2d_stage_plan([E[k] for k in classes])["blocks"] == 2
        close(E, F)
        c.close()
    assert out[0]["clock"] == out[4]["clock"]
    for k in X.classes_of(d):
        a0, s0, r0 = out[0][k]
        a4, s4, r4 = out[4][k]
        assert list(s0) == [1, 2, 3] == list(s4)
        avg = max(np.abs(a4[:, :, i] - a0[:, :, i]).max() / np.abs(a0[:, :, i]).max() for i in range(a0.shape[2]))
        rows = float((np.abs(r4 - r0) / np.abs(r0)).max())
        print("class %d: averages %.2e, residual rows %.2e" % (k, avg, rows))
        assert avg <= 1e-12 and rows <= 1e-11


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def refused(E, run_it, match):
    before = {c: e.download(hfx.DISU_UPTS0) for c, e in E.items()}
    with pytest.raises(hfx.HfxError, match=match) as err:
        run_it()
    assert "fused 0" in str(err.value), str(err.value)
    for c, e in E.items():
        assert np.array_equal(e.download(hfx.DISU_UPTS0), before[c])


def test_refused_with_the_option_off():
    """both messages of today, each naming fused 0, the state untouched"""
    d = X.load("mx_p3_n4")
    c0 = hfx.Context(0)
    classes, E, F, pairs, B = make(c0, d)
    blocks = [E[c] for c in classes]
    refused(E, lambda: hfx.run_steps_blocks(blocks, F, 1, fused=4), "several element blocks")
    close(E, F)
    q = X.quad_block(3, 17)
    e, faces = build(c0, q)
    refused({1: e}, lambda: hfx.run_steps_blocks([e], faces, 1, fused=4), "three-dimensional")
    for f in faces:
        f.close()
    e.close()
    c0.close()


@pytest.mark.parametrize("on", [X.TRI, X.QUAD])
def test_refused_features(ctx, on):
    """an LES closure, over-integration or shock capturing on either block: arrays of the right shape suffice, the refusal comes
    before anything reads them"""
    d = X.load("mx_p3_walls")
    for what in ("LES closure", "over-integration", "shock capturing"):
        classes, E, F, pairs, B = make(ctx, d)
        e = E[on]
        nu, nfp, ne = X.sizes(d, on)[1], X.sizes(d, on)[2], X.sizes(d, on)[0]
        if what == "LES closure":
            e.set_les(1, 0.325, 1.0, 0.41, 0.9, np.ones((2, 2, nfp, ne), order="F"))
        elif what == "over-integration":
            e.set_over_int(np.zeros((nu + 2, nu), order="F"), np.zeros((nu, nu + 2), order="F"), np.ones((2, 2, nu + 2, ne), order="F"))
        else:
            e.set_shock_capture(np.eye(nu, order="F"), np.eye(nu, order="F"), np.ones(nu), np.arange(nu - 1, nu, dtype=np.int32), 1.0, 0)
        refused(E, lambda: hfx.run_steps_blocks([E[c] for c in classes], F, 1, fused=4), what)
        close(E, F)


def test_refused_sizes_faces_and_loops(ctx):
    d = X.load("mx_p3_walls")
    # P5 quadrilaterals: 36 solution and 24 flux points do not fit (arrays of the right shape suffice)
    q = X.quad_block(3, 5)
    ne = int(q["sizes"][0])
    rng = np.random.default_rng(5)
    p5 = {k: v for k, v in q.items() if not k.startswith(("int", "bdy", "opp_"))}
    p5["sizes"] = np.array([ne, 36, 24] + [int(v) for v in q["sizes"][3:5]] + [5] + [int(v) for v in q["sizes"][6:]], dtype=np.int32)
    shape = {"opp_0": (24, 36), "opp_3": (36, 24), "opp_6": (24, 36)}
    for w in (1, 2, 4, 5):
        for dd in range(2):
            shape["opp_%d_%d" % (w, dd)] = {1: (24, 36), 2: (36, 36), 4: (36, 36), 5: (36, 24)}[w]
    for k, s in shape.items():
        p5[k] = np.asfortranarray(rng.standard_normal(s))
    p5["detjac_upts"] = np.ones((36, ne), order="F"); p5["detjac_fpts"] = np.ones((24, ne), order="F"); p5["tdA_fpts"] = np.ones((24, ne), order="F")
    p5["JGinv_upts"] = np.asfortranarray(np.tile(np.eye(2)[:, :, None, None], (1, 1, 36, ne)))
    p5["JGinv_fpts"] = np.asfortranarray(np.tile(np.eye(2)[:, :, None, None], (1, 1, 24, ne)))
    p5["norm_fpts"] = np.asfortranarray(np.tile(np.array([1.0, 0.0])[None, None, :], (24, ne, 1)))
    p5["u_init"] = np.asfortranarray(np.tile(q["u_init"][:1], (36, 1, 1)))
    ctx.set_params(hfx.params_from(p5))
    sz = [int(v) for v in p5["sizes"]]
    e = hfx.Eles(ctx, sz[:5], p5, ele_type=1, order=5)
    e.upload(hfx.DISU_UPTS0, p5["u_init"])
    refused({1: e}, lambda: hfx.run_steps_blocks([e], [], 1, fused=4), "quadrilaterals of orders 1..4")
    e.close()
    # a partition-face block: the triangles' boundary faces as one
    classes, E, F, pairs, B = make(ctx, d)
    blocks = [E[c] for c in classes]
    classes2, per, faces, bdy = MU.split(d)
    L = [Lb for a, Lb, ids in bdy if a == X.TRI][0]
    keep = [f for f, (a, Lb, ids) in zip(B, bdy) if not (a == X.TRI and Lb is L)]
    mpi = hfx.MpiInters(ctx, E[X.TRI], L, np.repeat(np.arange(L.shape[0], dtype=np.int32)[::-1, None], L.shape[1], axis=1))
    interior = F[:len(pairs)]
    refused(E, lambda: hfx.run_steps_blocks(blocks, interior + keep + [mpi], 1, fused=4), "partition-face block")
    mpi.close()
    # several two-dimensional blocks in the partitioned loop, the option on
    comm = hfx.Comm(ctx.h, hfx.comm_unique_id(), 1, 0)
    refused(E, lambda: hfx.run_steps_partitioned_blocks(blocks, F, [], comm, 1), "several element blocks")
    comm.close()
    # ... and the blocks run afterwards: a refusal leaves nothing behind
    hfx.run_steps_blocks(blocks, F, 1, fused=4)
    for c in classes:
        assert relerr(E[c].download(hfx.DISU_UPTS0), final_states(d)[0][c]["u"]) < TOL_U
    close(E, F)


def test_refused_orders_and_dimensions(ctx):
    """blocks of different order, and a three-dimensional block beside a two-dimensional one"""
    import os
    d3, d2 = X.load("mx_p3_n4"), X.load("mx_p2_n4")
    classes, E3, F3, pairs, B = make(ctx, d3)
    _, E2, F2, _, _ = make(ctx, d2)
    ctx.set_params(hfx.params_from(MU.split(d3)[1][0]))
    both = {0: E3[0], 1: E2[1]}
    refused(both, lambda: hfx.run_steps_blocks([E3[0], E2[1]], [], 1, fused=4), "different order")
    h = dict(np.load(os.path.join(os.path.dirname(X.GOLDEN), "hex_p2_n3_deformed.npz")))
    sz = [int(v) for v in h["sizes"]]
    e = hfx.Eles(ctx, sz[:5], h, ele_type=sz[6], order=sz[5])
    e.upload(hfx.DISU_UPTS0, h["u_init"])
    refused({0: E3[0]}, lambda: hfx.run_steps_blocks([E3[0], e], [], 1, fused=4), "three-dimensional block beside")
    e.close()
    close(E3, F3)
    close(E2, F2)
