"""The persistent element loops of the fused stages past their first iteration.

Every fused element kernel walks its elements in a software-pipelined loop (csrc/split3_kernels.hpp EleOrder, csrc/split2_kernels.hpp,
csrc/tensor_ops.hip), but a grid of min(n_eles, n_cu * per_cu) workgroups gives a mesh of a few dozen elements one element per
workgroup: the second LDS slot, the prefetch of the next element and of the partner words two ahead, the tail iteration and the
workgroup without work never run.  Option "persistent_grid_cap" launches every such kernel with at most n workgroups; here it
makes 27 hexes / 15 quads loop at caps 2, 3, 8 and 16:

    27 elements   cap 2: trips 14 / 13 (ragged, both slot parities)      cap 3: 9 / 9 / 9 (odd count)
                  cap 8: XCD remap on, chunk 4, workgroup 6 walks 3 elements, workgroup 7 none
                  cap 16: per = 2, workgroups 7 and 15 none, workgroup 14 one element and no next
    15 quads      cap 8: chunk 2, workgroup 7 one element           (cap 16 >= 15 elements is one element per workgroup: not run)

Nothing is judged against a capped run itself: the CPU oracle on the host mirror's registration (1e-11, as
test_gpu_host_mirror.py::test_mid_size_vs_oracle), the per-method path (1e-12, as test_split_paths_every_order_vs_methods), the
genuine reference's fixtures (1e-11) -- and the uncapped run of the same form, pinned by the rest of the suite, bit for bit: a cap
only moves elements between workgroups.  Every test asserts from the grids the library reports (hfx_fused_launch_grids) that its
kernels did loop."""
import ctypes as C
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
import oracle_py as O
import partition_util as PU
from test_gpu_affine_metrics import sheared_xv
from test_gpu_methods_vs_golden import build, relerr, GOLDEN

pytestmark = pytest.mark.gpu

SHAPE = {3: [3, 3, 3], 2: [5, 3, 1]}
CAPS = {3: (2, 3, 8, 16), 2: (2, 3, 8)}
TOL_ORACLE, TOL_METHODS, TOL_FIXTURE, TOL_PARTITION = 1e-11, 1e-12, 1e-11, 1e-11
ELEMENT, UPDATE, OVER_INT, SHOCK = 1, 3, 4, 5  # slots of hfx_fused_launch_grids


class _Ctx:
    """a bare handle with hfx.Context's methods (the host mirror owns the context)"""
    def __init__(self, h):
        self.h = h


def set_option(case, name, value):
    hfx.Context.set_option(_Ctx(case.handles()[0]), name, value)


# ---- what the library must report, and EleOrder restated ---------------------------------------------------------------

def ele_order(work, grid, remap_wanted):
    """the elements (or list positions) of every workgroup in the order it walks them: EleOrder (csrc/split3_kernels.hpp) when
    `remap_wanted` (all elements, option xcd_order on), else element = workgroup + k * grid"""
    if not (remap_wanted and grid % 8 == 0):
        return [list(range(b, work, grid)) for b in range(grid)]
    per, chunk = grid // 8, (work + 7) // 8
    return [[(b % 8) * chunk + l for l in range(b // 8, chunk, per) if (b % 8) * chunk + l < work] for b in range(grid)]


def check_loops(grids, cap, slots=None):
    """every element kernel launched: grid = min(work, cap), and at least 2 trips (3 at caps 2 and 3) for its busiest workgroup"""
    assert grids, "no persistent element kernel was launched"
    if slots is not None:
        assert sorted({s for s, _, _ in grids}) == sorted(slots), grids
    for slot, grid, work in grids:
        assert grid == min(work, cap), (slot, grid, work, cap)
        assert -(-work // grid) >= (3 if cap in (2, 3) else 2), (slot, grid, work, cap)
        for remap in (False, True):  # (the restatement deals every element exactly once)
            assert sorted(sum(ele_order(work, grid, remap), [])) == list(range(work))


def check_remapped_workgroups(grids, cap, slots):
    """caps 8 and 16 on all elements with the XCD order on: the workgroups without work and the short ones (module docstring)"""
    for slot, grid, work in grids:
        if slot not in slots or cap not in (8, 16):
            continue
        n = [len(w) for w in ele_order(work, grid, True)]
        empty = [b for b, k in enumerate(n) if k == 0]
        if (work, cap) == (27, 8):
            assert empty == [7] and n[6] == 3 and n[:6] == [4] * 6
        elif (work, cap) == (27, 16):
            assert empty == [7, 15] and n[14] == 1 and n[6] == 2
        elif (work, cap) == (15, 8):
            assert empty == [] and n[7] == 1 and n[:7] == [2] * 7
        else:
            raise AssertionError("no table for %d elements at cap %d" % (work, cap))


def test_ele_order_restated_gives_the_trip_counts_of_the_table():
    """(no GPU work: the numpy restatement against the table of the module docstring)"""
    assert [len(w) for w in ele_order(27, 2, True)] == [14, 13]
    assert [len(w) for w in ele_order(27, 3, True)] == [9, 9, 9]
    check_remapped_workgroups([(ELEMENT, 8, 27), (ELEMENT, 8, 15)], 8, (ELEMENT,))
    check_remapped_workgroups([(ELEMENT, 16, 27)], 16, (ELEMENT,))
    assert ele_order(27, 8, True)[6] == [24, 25, 26] and ele_order(27, 16, True)[14] == [25]


# ---- cases, references (computed once, never written to) --------------------------------------------------------------------

def case_kw(dims, order, mesh):
    """mesh: "deformed" (amp 0.1), "box" (amp 0: an affine block), "sheared" (the affine box of test_gpu_affine_metrics.py)"""
    kw = dict(dims=dims, order=order) if dims == 2 else dict(order=order)
    if mesh == "deformed":
        kw["amp"] = 0.1
    elif mesh == "sheared":
        kw["xv"] = sheared_xv(SHAPE[dims], dims)
    return kw


def run(dims, order, mesh, fused, steps, opts=(), cap=0):
    """the state after each step (each its own hfx_run_steps call) and the launch grids of the last stage"""
    c = H.Case(SHAPE[dims], **case_kw(dims, order, mesh))
    c.to_device(0)
    for k, v in opts:
        set_option(c, k, v)
    if cap:
        set_option(c, "persistent_grid_cap", cap)
    out = []
    for _ in range(steps):
        c.run_steps_lib(1, fused=fused)
        c.sync_host()
        out.append(c.array("disu_upts0").copy())
    grids = hfx.fused_launch_grids(c.handles()[1]) if fused else []
    c.close()
    return out, grids


_REFS = {}


def references(dims, order, mesh):
    """(the oracle's state, the per-method path's state) after ONE RK step, and the initial state"""
    key = (dims, order, mesh)
    if key not in _REFS:
        c = H.Case(SHAPE[dims], **case_kw(dims, order, mesh))
        u_init = c.array("disu_upts0").copy()
        oc = O.Case(c.registration())
        c.close()
        orc = O.load()
        e = oc.c_eles()
        f, nb = oc.c_faces()
        orc.orc_set_threads(8)
        bad = orc.orc_rk_step(C.byref(e), f, nb, C.byref(oc.params))
        orc.orc_set_threads(1)
        assert bad == -1
        methods = run(dims, order, mesh, False, 1)[0][0]
        for a in (oc.arr["u0"], methods, u_init):
            a.setflags(write=False)
        _REFS[key] = (oc.arr["u0"], methods, u_init)
    return _REFS[key]


def check_capped_against_everything(dims, order, mesh, mode, caps, opts=(), exact=True, slots=(ELEMENT, UPDATE), remapped=None):
    """Two steps under every cap of `caps`: the first against the oracle and the per-method path, both against the uncapped
    run of the same form (bits when `exact`); the launch grids against check_loops and, for the kernels `remapped` names, the table"""
    want_oracle, want_methods, u_init = references(dims, order, mesh)
    free, g0 = run(dims, order, mesh, mode, 2, opts)
    n_eles = int(np.prod(SHAPE[dims]))
    assert all(grid == work == n_eles for _, grid, work in g0), g0  # (uncapped: one element per workgroup, as ever)
    assert relerr(free[0], u_init) > 1e-8  # (the state moved)
    for cap in caps:
        got, grids = run(dims, order, mesh, mode, 2, opts, cap)
        print("dims %d P%d %s mode %s %s cap %d: grids %s, vs oracle %.3g, vs methods %.3g, vs uncapped %.3g" %
              (dims, order, mesh, mode, list(opts), cap, grids, relerr(got[0], want_oracle), relerr(got[0], want_methods), relerr(got[1], free[1])))
        check_loops(grids, cap, slots)
        assert [g[2] for g in grids] == [n_eles] * len(grids)
        if remapped:
            check_remapped_workgroups(grids, cap, remapped)
        assert relerr(got[0], want_oracle) < TOL_ORACLE, cap
        assert relerr(got[0], want_methods) < TOL_METHODS, cap
        for s in range(2):
            if exact:
                assert np.array_equal(got[s], free[s]), (cap, s)
            else:
                assert relerr(got[s], free[s]) < TOL_METHODS, (cap, s)


# ---- every element size ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("dims", [2, 3])
def test_every_element_size_loops(dims, order, mode):
    """Every instantiated element size of variant 2 (gradient and residual kernels) and variant 3 (flux and update kernels, with
    the loader wave or the register pipeline, whichever the size selects; hexes P6 and P7 run variant 2 when 3 is asked for)
    at every cap.  The flux and update kernels of variant 3 walk EleOrder: their empty and short workgroups at caps 8 and 16
    are asserted; variant 2 strides by the grid."""
    v3 = mode == 3 and not (dims == 3 and order > 5)
    check_capped_against_everything(dims, order, "deformed", mode, CAPS[dims], remapped=(ELEMENT, UPDATE) if v3 else None)


# ---- every form of the split3 kernels ----------------------------------------------------------------------------------------

FORMS = [("loader_wave", 0), ("gather_delta", 0), ("flux_waves", 3), ("buffer_addressing", 0), ("dictionary_rows", 1),
         ("simd_roles", 0), ("light_wave_short", 0), ("xcd_order", 0)]


@pytest.mark.parametrize("knob,value", FORMS)
@pytest.mark.parametrize("dims,order", [(3, 4), (3, 2), (2, 3)])
def test_every_form_of_the_split3_kernels_loops(dims, order, knob, value):
    """One option of the split3 kernels at a time (register pipeline with 2 and 3 waves, flat addressing, dictionary rows, the
    pairwise LDG kernel in place of the gathered corrections, waves dealt by number, the paired form on the light wave, the
    plain element order), caps 3 and 8.  Each form against the oracle and the per-method path, and bit for bit against ITS
    uncapped run."""
    # (the dictionary-row flux kernel strides by the grid; with xcd_order 0 nothing is remapped)
    remapped = None if knob == "xcd_order" else (UPDATE,) if knob == "dictionary_rows" else (ELEMENT, UPDATE)
    check_capped_against_everything(dims, order, "deformed", 3, (3, 8), opts=[(knob, value)], remapped=remapped)


@pytest.mark.parametrize("affine", [0, 1])
@pytest.mark.parametrize("mesh", ["box", "sheared"])
@pytest.mark.parametrize("dims,order", [(3, 4), (3, 2), (2, 3)])
def test_affine_blocks_loop(dims, order, mesh, affine):
    """The per-element metric record (aff_rec[e]) for elements beyond a workgroup's first, and the general-metric loader wave on
    the same affine meshes (affine_metrics 0)."""
    check_capped_against_everything(dims, order, mesh, 3, (3, 8), opts=[("affine_metrics", affine)], remapped=(ELEMENT, UPDATE))


# ---- ingredients, against the genuine reference's fixtures --------------------------------------------------------------------

def fixture_caps(d):
    """caps 3 and 8 -- but a fixture of 8 elements has one element per workgroup at cap 8 (hex_p4_jet, hex_p6_deformed): those run
    caps 2 and 3"""
    return (3, 8) if int(d["sizes"][0]) > 8 else (2, 3)


INGREDIENTS = [("hex_p2_overint", ("over_int_fold", 1)), ("hex_p2_overint", ("over_int_fold", 0)),
               ("quad_p3_overint", ("over_int_fold", 1)), ("quad_p3_overint", ("over_int_fold", 0)),
               ("hex_p3_shock", None), ("quad_p3_shock", None), ("hex_p4_jet", None),
               ("hex_p2_les_wale", None), ("quad_p3_les_wale", None),
               ("hex_p4_n3_deformed", None), ("hex_p3_n3_deformed", None), ("hex_p2_n3_deformed", None),
               ("hex_p6_deformed", None), ("quad_p7_deformed", None)]


@pytest.mark.parametrize("name,opt", INGREDIENTS)
def test_ingredients_loop_vs_reference(name, opt):
    """test_gpu_fused.py::test_fused_vs_reference (variant 3) under a cap: the sum-factorised over-integration kernel, folded and
    not, the shock-capturing kernel behind the update, the LES closure inside the flux kernel, boundary faces (hex_p4_jet),
    every step of the fixture at its tolerance."""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    nstage = int(d["sizes"][7])
    steps = sorted({int(k.split("_")[1][4:]) for k in d if k.startswith("u_step")})
    # (the sum-factorised over-integration and shock-capturing kernels where the fixture has the ingredient: build() registers it)
    slots = {ELEMENT, UPDATE}
    if "over_int" in d and int(np.ravel(d["over_int"])[0]):
        slots.add(OVER_INT)
    if "shock_cap" in d and int(np.ravel(d["shock_cap"])[0]):
        slots.add(SHOCK)
    assert ("overint" in name) <= (OVER_INT in slots) and ("shock" in name) <= (SHOCK in slots)
    for cap in fixture_caps(d):
        ctx = hfx.Context(0)
        e, faces = build(ctx, d)
        if opt:
            ctx.set_option(*opt)
        ctx.set_option("persistent_grid_cap", cap)
        for st in steps:
            hfx.run_steps(e, faces, 1, fused=3)
            err = relerr(e.download(hfx.DISU_UPTS0), d["u_step%d_stage%d" % (st, nstage - 1)])
            print("%s %s cap %d step %d: vs reference %.3g" % (name, opt, cap, st, err))
            assert err < TOL_FIXTURE, (cap, st)
        assert e.check_nan() == -1
        grids = hfx.fused_launch_grids(e.h)
        print("%s cap %d: grids %s" % (name, cap, grids))
        check_loops(grids, cap, slots)
        for f in faces:
            f.close()
        e.close()
        ctx.close()


# ---- element lists on partitioned blocks ---------------------------------------------------------------------------------------

PART_CFG = dict(amp=0.05, length=6.2831853071795862, T_c_ic=300.0, dt=1e-4, riemann_solve_type=3)
PART_N = [5, 3, 3]  # wrap-around faces of x as partition faces: 18 elements with partition-face points, 27 without (13 + 14)


def _lists_worker(rank, world, port, outdir, order, opts):
    import torch
    torch.cuda.set_device(0)
    c = H.Case(PART_N, self_partition=[1, 0, 0], order=order, **PART_CFG)
    c.to_device(0)
    for k, v in opts:
        set_option(c, k, v)
    set_option(c, "persistent_grid_cap", 2)
    c.set_comm(hfx.comm_unique_id())
    c.run_partitioned(2)
    c.sync_host()
    np.save(outdir + "/u.npy", c.array("disu_upts0"))
    np.save(outdir + "/grids.npy", np.array(hfx.fused_launch_grids(c.handles()[1]), dtype=np.int64))
    c.close()


@pytest.mark.parametrize("opts", [(), (("split_flux", 0),), (("split_update", 0),)])
@pytest.mark.parametrize("order", [4, 2])
def test_element_lists_loop(tmp_path, order, opts):
    """A self-partitioned block over the library's RCCL transport, cap 2: the flux kernel on the two halves of the elements
    without partition-face points and on those with, the update kernel on the two lists -- EleOrder::at through an element
    list, 7 to 9 trips per workgroup -- against the undivided box's oracle.  split_flux 0 / split_update 0: that kernel in one
    launch on all 45 elements beside the other's lists."""
    PU.spawn(_lists_worker, 1, (str(tmp_path), order, opts))
    grids = [tuple(int(v) for v in g) for g in np.load(str(tmp_path / "grids.npy"))]
    print("P%d %s: grids %s" % (order, opts, grids))
    check_loops(grids, 2, (ELEMENT, UPDATE))
    want = {ELEMENT: [13, 18, 14], UPDATE: [18, 27]}  # interior_1, partition, interior_2 | partition, interior
    if ("split_flux", 0) in opts:
        want[ELEMENT] = [45]
    if ("split_update", 0) in opts:
        want[UPDATE] = [45]
    for slot in (ELEMENT, UPDATE):
        work = [w for s, _, w in grids if s == slot]
        assert work == want[slot], (slot, work)
        assert min(work) > 2 and len(set(work)) == len(work)  # (each list longer than the cap, all of different lengths)
    u1, _ = PU.single_rank_oracle(PART_N, dict(PART_CFG, order=order), 2)
    assert relerr(np.load(str(tmp_path / "u.npy")), u1) < TOL_PARTITION


@pytest.mark.parametrize("order", [4, 2])
def test_two_rank_partitioned_block_loops(order):
    """Two ranks as threads of this process (partition_util.ThreadTransport), cap 2 on each rank's 27 elements: the partitioned
    stage with the caller's transport launches its element kernels on all elements of the rank."""
    import threading
    import torch
    n_local, pgrid, cfg = [3, 3, 3], [2, 1, 1], dict(PART_CFG, order=order)
    torch.cuda.set_device(0)
    T = PU.ThreadTransport(2)
    out, err = [None, None], []

    def work(rank):
        try:
            torch.cuda.set_device(0)
            c = H.Case(n_local, rank=rank, pgrid=pgrid, **cfg)
            c.to_device(0)
            set_option(c, "persistent_grid_cap", 2)
            T.register(rank, c, projected_flux=True)
            c.set_exchange(T.hook(rank))
            c.set_reduce_min(T.reduce_min(rank))
            T.barrier.wait()
            c.run_partitioned(2)
            c.sync_host()
            out[rank] = (c.array("disu_upts0"), hfx.fused_launch_grids(c.handles()[1]))
            T.barrier.wait()
            c.close()
        except BaseException as e:  # noqa: BLE001
            err.append(e)
            T.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if err:
        raise err[0]
    for u, grids in out:
        print("P%d: grids %s" % (order, grids))
        check_loops(grids, 2, (ELEMENT, UPDATE))
    u1, _ = PU.single_rank_oracle([6, 3, 3], cfg, 2)
    u = PU.assemble_arrays(out, 0, n_local, pgrid, u1.shape)
    assert relerr(u, u1) < TOL_PARTITION


# ---- the deferred path -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,order", [(3, 4), (2, 3)])
def test_deferred_mirrored_loop_loops(dims, order):
    """The host mirror's unchanged CalcResidual / AdvanceSolution loop with cap 3: every stage still runs as a fused stage (the
    state alone is read, so the stage pending at the end runs fused for it), on capped grids, and gives the oracle's and the
    per-method path's state."""
    want_oracle, want_methods, u_init = references(dims, order, "deformed")
    c = H.Case(SHAPE[dims], **case_kw(dims, order, "deformed"))
    c.to_device(0)
    set_option(c, "persistent_grid_cap", 3)
    c.run(1)
    ctx, e = c.handles()[0], c.handles()[1]
    u = np.zeros(u_init.shape, order="F")
    hfx.check(hfx.lib().hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u.ctypes.data_as(hfx.dp)))
    nf, nr, why = hfx.deferred_stats(ctx)
    grids = hfx.fused_launch_grids(e)
    c.close()
    print("dims %d P%d deferred: grids %s, vs oracle %.3g, vs methods %.3g" % (dims, order, grids, relerr(u, want_oracle), relerr(u, want_methods)))
    assert (nf, nr) == (c.n_stages, 0), why
    check_loops(grids, 3, (ELEMENT, UPDATE))
    assert relerr(u, want_oracle) < TOL_ORACLE
    assert relerr(u, want_methods) < TOL_METHODS
