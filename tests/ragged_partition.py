"""Ragged, graph-like partitions cut in test code: TEST INFRASTRUCTURE.

The host mirror splits a box into equal blocks on a process grid (partition_util.py).  A k-way graph partition looks
different: parts of unequal size, many neighbours with segments of unequal length, elements with several faces on one
neighbour, parts without a single element free of partition-face points.  `cut` makes such a partition out of the
registration dict of the UNDIVIDED mesh and a per-element part vector; `cut_self` keeps all elements on one rank and
turns the faces between virtual parts into partition faces whose neighbour is the rank itself.  The tables follow the
convention include/hfx.h states for hfx_mpi_inters_create / hfx_mpi_inters_set_neighbours:

  - faces of one neighbour are contiguous, neighbours in ascending rank order;
  - within a pair of ranks the faces keep the order of the undivided face table, so both ranks list them alike;
  - the side that was LEFT in the undivided table lists its points as that table does, the side that was RIGHT lists its
    own points in ascending offset; Rlut[j, i] is the slot, in the peer's record of face i, of the point that meets j.

The lockstep drivers run all parts in one process and one thread: every part advances to the next point where the
reference starts or awaits a message, then the records are moved (numpy on the CPU, device-to-device copies on the GPU).
"""
import ctypes as C

import numpy as np

# arrays of a registration dict that carry an element axis, and which one: (pt, ele, ...) or (dim, dim, pt, ele)
ELEMENT_AXIS = {"detjac_upts": 1, "detjac_fpts": 1, "tdA_fpts": 1, "norm_fpts": 1, "u_init": 1, "wall_distance": 1,
                "JGinv_upts": 3, "JGinv_fpts": 3, "Jacobian_fpts": 3, "JGinv_over_int_cubpts": 3}


def F32(a):
    return np.asfortranarray(np.array(a, dtype=np.int32))


# ---- part vectors ------------------------------------------------------------------------------------------------------------

def grow_parts(n, weights, seed):
    """Seeded part vector of the periodic box of n[0] x n[1] x n[2] elements (x fastest): every part grows from a random seed
    element by a random walk over face neighbours until it holds its share `weights` of the elements; what no walk reached
    goes to the neighbouring part that comes first."""
    rng = np.random.RandomState(seed)
    n = list(n)
    ne = int(np.prod(n))
    w = np.array(weights, dtype=np.float64)
    target = np.maximum(1, np.floor(w / w.sum() * ne).astype(int))

    def neighbours(el):
        c = [el % n[0], (el // n[0]) % n[1], el // (n[0] * n[1])]
        out = []
        for d in range(3):
            for s in (-1, 1):
                q = list(c)
                q[d] = (q[d] + s) % n[d]
                out.append(q[0] + n[0] * (q[1] + n[1] * q[2]))
        return out

    part = -np.ones(ne, dtype=np.int64)
    seeds = rng.choice(ne, size=len(w), replace=False)
    at = list(seeds)
    for p, s in enumerate(seeds):
        part[s] = p
    size = np.ones(len(w), dtype=int)
    for _ in range(200 * ne):
        open_parts = [p for p in range(len(w)) if size[p] < target[p]]
        if not open_parts or (part >= 0).all():
            break
        p = open_parts[rng.randint(len(open_parts))]
        free = [q for q in neighbours(at[p]) if part[q] < 0]
        if free:
            at[p] = free[rng.randint(len(free))]
            part[at[p]] = p
            size[p] += 1
        else:  # walk on inside the part
            own = [q for q in neighbours(at[p]) if part[q] == p]
            at[p] = own[rng.randint(len(own))] if own else int(rng.choice(np.flatnonzero(part == p)))
    while (part < 0).any():
        for el in np.flatnonzero(part < 0):
            near = [part[q] for q in neighbours(el) if part[q] >= 0]
            if near:
                part[el] = near[0]
    return part


# ---- the cut ------------------------------------------------------------------------------------------------------------------

def face_types(reg, kind="int"):
    return [t for t in range(3) if "%s%d_L" % (kind, t) in reg]


def peer_points(R):
    """(order, slot, Lb) of a block of faces from the right sides' offsets R: Lb = the right side's own record (its points in
    ascending offset), order[j', i] = the left point whose partner is the right side's j'-th point, slot[j, i] = where left
    point j's partner sits in the right side's record"""
    order = np.argsort(R, axis=0, kind="stable")
    slot = np.argsort(order, axis=0, kind="stable")
    return order, slot, np.take_along_axis(R, order, axis=0)


class Part:
    """one part of a cut: reg (registration dict of its elements, interior and boundary tables included), elems (global
    element numbers, ascending), L / Rlut (partition-face table), segments [(peer, send_first, recv_first, count)],
    faces (for every partition face: index into the undivided table, 1 if this part is the table's left side)"""


def cut(reg, part):
    """-> [Part] of the one-block registration dict `reg` under the per-element part vector `part`"""
    part = np.asarray(part)
    sz = [int(v) for v in reg["sizes"]]
    ne, nfp = sz[0], sz[2]
    assert part.shape == (ne,) and part.min() == 0
    n_parts = int(part.max()) + 1
    tt = face_types(reg)
    assert len(tt) == 1, "one face type per block"
    t = tt[0]
    L, R = np.asarray(reg["int%d_L" % t]), np.asarray(reg["int%d_R" % t])
    pl, pr = part[L[0] // nfp], part[R[0] // nfp]
    order, slot, Lb = peer_points(R)
    local = np.zeros(ne, dtype=np.int64)
    out = []
    for p in range(n_parts):
        P = Part()
        P.elems = np.flatnonzero(part == p)
        assert P.elems.size, "part %d is empty" % p
        local[:] = -1
        local[P.elems] = np.arange(P.elems.size)

        def renum(tab):
            r = tab % nfp + nfp * local[tab // nfp]
            assert (local[tab // nfp] >= 0).all()
            return F32(r)

        d = {k: v for k, v in reg.items() if not k.startswith(("int", "bdy"))}
        for k, axis in ELEMENT_AXIS.items():
            if k in d:
                d[k] = np.asfortranarray(np.take(d[k], P.elems, axis=axis))
        d["sizes"] = np.array([P.elems.size] + sz[1:], dtype=np.int32)
        keep = (pl == p) & (pr == p)
        d["int%d_L" % t], d["int%d_R" % t] = renum(L[:, keep]), renum(R[:, keep])
        for tb in face_types(reg, "bdy"):
            bL, ids = np.asarray(reg["bdy%d_L" % tb]), np.ravel(reg["bdy%d_id" % tb])
            m = part[bL[0] // nfp] == p
            if m.any():
                d["bdy%d_L" % tb], d["bdy%d_id" % tb] = renum(bL[:, m]), np.ascontiguousarray(ids[m].astype(np.int32))
        P.reg = d
        cols, luts, P.segments, P.faces = [], [], [], []
        first = 0
        for q in range(n_parts):
            if q == p:
                continue
            idx = np.flatnonzero(((pl == p) & (pr == q)) | ((pl == q) & (pr == p)))  # the pair's faces in table order
            if not idx.size:
                continue
            for i in idx:
                left = pl[i] == p
                cols.append(L[:, i] if left else Lb[:, i])
                luts.append(slot[:, i] if left else order[:, i])
                P.faces.append((int(i), int(left)))
            P.segments.append((q, first, first, int(idx.size)))
            first += int(idx.size)
        P.L = renum(np.stack(cols, axis=1)) if cols else np.zeros((L.shape[0], 0), dtype=np.int32, order="F")
        P.Rlut = F32(np.stack(luts, axis=1)) if cols else P.L.copy(order="F")
        out.append(P)
    return out


def cut_faces_self(faces, labels):
    """The cut for ONE rank that keeps all elements.  faces: [(a, b, L, R)] interior blocks between element blocks a and b
    (mixed_util.split's form); labels(a, b, L, R) -> None (the block stays whole) or (va, vb): the virtual part of the left
    and of the right side of every face.  Faces with va != vb become pairs of one-sided partition faces whose peer is rank 0.
    -> (remaining interior blocks, [(a, Lm, Rlut, segments)]): per block one directed segment for every ordered pair of
    virtual parts (ascending), the faces of a pair in table order in both of its segments; recv_first of a segment is where
    its MATE's faces sit -- comm.hip matches a rank's sends to itself with its receives segment by segment in posting order,
    so what segment s sends has to land where the faces of the other side read."""
    rest, mpi = [], []
    for a, b, L, R in faces:
        lab = labels(a, b, L, R)
        if lab is None:
            rest.append((a, b, L, R))
            continue
        va, vb = (np.asarray(v) for v in lab)
        same = va == vb
        if same.all():
            rest.append((a, b, L, R))
            continue
        if not same.all() and same.any():
            rest.append((a, b, np.asfortranarray(L[:, same]), np.asfortranarray(R[:, same])))
        order, slot, Lb = peer_points(R)
        pairs = sorted({(int(x), int(y)) for x, y in zip(va[~same], vb[~same])} | {(int(y), int(x)) for x, y in zip(va[~same], vb[~same])})
        cols, luts, first, count = [], [], {}, {}
        n = 0
        for x, y in pairs:
            idx = np.flatnonzero(((va == x) & (vb == y)) | ((va == y) & (vb == x)))
            for i in idx:
                left = va[i] == x
                cols.append(L[:, i] if left else Lb[:, i])
                luts.append(slot[:, i] if left else order[:, i])
            first[(x, y)], count[(x, y)] = n, int(idx.size)
            n += int(idx.size)
        seg = [(0, first[(x, y)], first[(y, x)], count[(x, y)]) for x, y in pairs]
        mpi.append((a, F32(np.stack(cols, axis=1)), F32(np.stack(luts, axis=1)), seg))
    return rest, mpi


def part_labels(part, n_fpts):
    """labels for cut_faces_self from per-element part vectors: part = {block: vector}, n_fpts = {block: flux points per
    element}; only faces that join a block to itself are cut"""
    def labels(a, b, L, R):
        if a != b or a not in part:
            return None
        return part[a][L[0] // n_fpts[a]], part[a][R[0] // n_fpts[a]]
    return labels


def every_second_face(a, b, L, R):
    """the rule of the self-partitioned mixed-channel tests: of every block that joins a class to itself (4 faces or more),
    faces 0, 2, 4, ... -- left sides virtual part 0, right sides virtual part 1"""
    if a != b or L.shape[1] < 4:
        return None
    vb = np.zeros(L.shape[1], dtype=np.int64)
    vb[::2] = 1
    return np.zeros(L.shape[1], dtype=np.int64), vb


def cut_self(blocks, part):
    """`cut` for a single rank that keeps all elements.  blocks: a one-block registration dict (part: the part vector) -> (the
    dict with the remaining interior faces, L, Rlut, segments); or mixed_util.split's (classes, per, faces, bdy) (part: {class:
    vector}) -> (remaining interior blocks, [(class, L, Rlut, segments)])"""
    if isinstance(blocks, dict):
        nfp = int(blocks["sizes"][2])
        t = face_types(blocks)[0]
        rest, mpi = cut_faces_self([(0, 0, np.asarray(blocks["int%d_L" % t]), np.asarray(blocks["int%d_R" % t]))],
                                   part_labels({0: np.asarray(part)}, {0: nfp}))
        d = dict(blocks)
        d["int%d_L" % t], d["int%d_R" % t] = F32(rest[0][2]), F32(rest[0][3])
        return (d,) + mpi[0][1:]
    classes, per, faces, bdy = blocks
    return cut_faces_self(faces, part_labels({c: np.asarray(v) for c, v in part.items()}, {c: int(per[c]["sizes"][2]) for c in classes}))


def self_partition(ctx, E, faces):
    """Every second face of every interior block that joins a class to ITSELF becomes a pair of one-sided partition faces whose
    neighbour is the rank itself: -> (remaining interior blocks as (a, b, L, R), [hfx.MpiInters]).  The partition-face block
    of a (class, face type) lists the left sides A_0..A_n-1, then the right sides B_0..B_n-1 (in the order of their own
    offsets); Rlut is the slot of the partner's point in the mate's record; the two halves are each other's neighbour segment."""
    import hfx
    rest, tabs = cut_faces_self(faces, every_second_face)
    mpi = []
    for a, Lm, Rlut, seg in tabs:
        f = hfx.MpiInters(ctx, E[a], Lm, Rlut)
        f.set_neighbours(seg)
        mpi.append(f)
    return rest, mpi


# ---- moving the records --------------------------------------------------------------------------------------------------------

def mate(segments, rank, s):
    """(owner, send_first) of what lands in segment s of `rank`: the peer's segment for this rank, or -- a rank's faces with
    itself -- this very segment (its k-th send meets its k-th receive)"""
    p = segments[rank][s][0]
    if p == rank:
        return p, segments[rank][s][1]
    m = [q for q in segments[p] if q[0] == rank]
    assert len(m) == 1 and m[0][3] == segments[rank][s][3]
    return p, m[0][1]


def move_records(segments, out, inn, rec):
    """out / inn: per rank a flat buffer (numpy array or torch tensor) of face records of `rec` doubles"""
    for r, segs in enumerate(segments):
        for s, (p, _, recv, count) in enumerate(segs):
            owner, send = mate(segments, r, s)
            inn[r][recv * rec:(recv + count) * rec] = out[owner][send * rec:(send + count) * rec]


def lockstep(points, move):
    """points: one generator per part, all yielding the same (kind, phase) sequence; move(kind) before anyone goes on past a
    phase-1 point.  -> what the generators returned"""
    done = [None] * len(points)
    while True:
        at = []
        for i, g in enumerate(points):
            try:
                at.append(next(g))
            except StopIteration as stop:
                at.append(None)
                done[i] = stop.value
        assert all(a == at[0] for a in at), at
        if at[0] is None:
            return done
        if at[0][1] == 1:
            move(at[0][0])


# ---- the oracle in lockstep ----------------------------------------------------------------------------------------------------

KIND_BUF = {0: ("out_disu", "in_disu"), 1: ("out_grad", "in_grad"), 2: ("out_sgsf", "in_sgsf")}


def oracle_lockstep(tables, n_steps):
    """tables: per rank (reg, L, Rlut, segments).  -> [oracle_py.PartitionedCase] after n_steps time steps"""
    import oracle_py as O
    O.load().orc_set_threads(1)
    cases = [O.PartitionedCase(reg, L, Rlut) for reg, L, Rlut, _ in tables]
    segments = [t[3] for t in tables]

    def move(kind):
        o, i = KIND_BUF[kind]
        recs = [c.buf[o].size // max(1, c.mL.shape[1]) for c in cases]
        assert len(set(recs)) == 1
        move_records(segments, [c.buf[o] for c in cases], [c.buf[i] for c in cases], recs[0])

    for _ in range(n_steps):
        lockstep([c.rk_step_points() for c in cases], move)
    return cases


def part_tables(parts):
    return [(P.reg, P.L, P.Rlut, P.segments) for P in parts]


def assemble(parts, arrays, shape):
    """the parts' (pt, ele, field) arrays put back in global element order"""
    out = np.zeros(shape, order="F")
    for P, a in zip(parts, arrays):
        out[:, P.elems, :] = a
    return out


def undivided_oracle(reg, n_steps):
    """(u, div) of the one-rank oracle on the whole registration dict, boundary blocks included"""
    import oracle_py as O
    o = O.load()
    oc = O.Case(reg)
    e, (f, nb) = oc.c_eles(), oc.c_faces()
    for _ in range(n_steps):
        if oc.bdy:
            b, nbd = oc.c_bdy()
            bad = o.orc_rk_step_bdy(C.byref(e), f, nb, b, nbd, C.byref(oc.params))
        else:
            bad = o.orc_rk_step(C.byref(e), f, nb, C.byref(oc.params))
        assert bad < 0
    return oc.arr["u0"], oc.arr["div_tconf_upts"]


# ---- libhfx in lockstep --------------------------------------------------------------------------------------------------------

class GpuPart:
    """one rank's blocks through the raw C ABI, in a context of its own on device 0"""

    def __init__(self, reg, L, Rlut, segments, fused_mode=None, options=()):
        import torch
        import exchange
        import hfx
        self.ctx = hfx.Context(0)
        self.ctx.set_params(hfx.params_from(reg))
        if fused_mode is not None:
            self.ctx.set_fused_mode(fused_mode)
        for k, v in options:
            self.ctx.set_option(k, v)
        sz = [int(v) for v in reg["sizes"]]
        self.e = hfx.Eles(self.ctx, sz[:5], reg, ele_type=sz[6], order=sz[5])
        self.e.upload(hfx.DISU_UPTS0, reg["u_init"])
        self.ints, self.bdys = [], []
        for t in face_types(reg):
            if np.asarray(reg["int%d_L" % t]).shape[1]:
                self.ints.append(hfx.IntInters(self.ctx, self.e, self.e, reg["int%d_L" % t], reg["int%d_R" % t]))
        for t in face_types(reg, "bdy"):
            self.bdys.append(hfx.BdyInters(self.ctx, self.e, reg["bdy%d_L" % t], reg["bdy%d_id" % t],
                                           hfx.bc_records(reg["bc_flags"], reg["bc_params"]), float(np.ravel(reg["bc_R_ref"])[0]),
                                           int(np.ravel(reg["ramp_counter"])[0])))
        self.m = hfx.MpiInters(self.ctx, self.e, L, Rlut)
        self.m.set_neighbours(segments)
        self.n_faces = int(np.asarray(L).shape[1])
        self.params = self.ctx.params
        dev = torch.device("cuda", 0)
        self.buf = {w: exchange.device_tensor(*hfx.mpi_buffer(self.m.h, w), dev) for w in range(6)}

    def methods_points(self, n_steps):
        """the per-method entry points in CalcResidual's order (src/solver.cpp:59-221), the packing halves of send_* and the
        one-sided calculate_common_*; yields like oracle_py.PartitionedCase.residual_points"""
        e, m, p = self.e, self.m, self.params
        for _ in range(n_steps):
            for rk in range(p.n_rk if p.adv_type else 1):
                e.extrapolate_solution()
                m.pack_solution()
                yield (0, 0)
                if p.viscous:
                    e.calculate_gradient()
                e.evaluate_invFlux()
                for f in self.ints: f.calculate_common_invFlux()
                for f in self.bdys: f.evaluate_boundaryConditions_invFlux()
                yield (0, 1)
                m.calculate_common_invFlux()
                if p.viscous:
                    e.correct_gradient()
                    m.pack_corrected_gradient()
                    yield (1, 0)
                    e.evaluate_viscFlux()
                e.extrapolate_totalFlux()
                e.calculate_divergence()
                if p.viscous:
                    for f in self.ints: f.calculate_common_viscFlux()
                    for f in self.bdys: f.evaluate_boundaryConditions_viscFlux()
                    yield (1, 1)
                    m.calculate_common_viscFlux()
                e.calculate_corrected_divergence()
                e.AdvanceSolution(rk, p.adv_type)

    def fused_points(self, n_steps):
        """hfx_stage_partitioned phases 0-4 as the host mirror's RunStepsPartitionedFused calls them"""
        import hfx
        p = self.params
        fi = [f.h for f in self.ints + self.bdys]
        fm = [self.m.h]
        first = True
        for _ in range(n_steps):
            for rk in range(p.n_rk if p.adv_type else 1):
                if first:
                    hfx.stage_partitioned(self.e.h, fi, fm, 0, rk, 1)
                    yield (0, 0)
                    first = False
                hfx.stage_partitioned(self.e.h, fi, fm, 1, rk, 0)
                yield (0, 1)
                hfx.stage_partitioned(self.e.h, fi, fm, 2, rk, 0)
                if p.viscous:
                    yield (1, 0)
                hfx.stage_partitioned(self.e.h, fi, fm, 3, rk, 0)
                if p.viscous:
                    yield (1, 1)
                hfx.stage_partitioned(self.e.h, fi, fm, 4, rk, 0)
                yield (0, 0)
        yield (0, 1)  # the message started after the last stage belongs to a stage that is not run: complete it

    def close(self):
        self.buf = {}
        for f in self.ints + self.bdys + [self.m]:
            f.close()
        self.e.close()
        self.ctx.close()


def gpu_lockstep(tables, n_steps, mode, options=()):
    """tables as for oracle_lockstep; mode "methods" | "fused" (fused mode 3, the projected flux in buffers 4/5 as the second
    message) | "fused2" (fused mode 2, the corrected gradient in buffers 2/3).  -> [(u, div)] per rank, and the ranks'
    hfx_fused_launch_grids"""
    import torch
    import hfx
    torch.cuda.set_device(0)
    ranks = [GpuPart(*t, fused_mode={"fused2": 2, "fused": 3}.get(mode), options=options) for t in tables]
    try:
        segments = [t[3] for t in tables]
        which = {0: (0, 1), 1: (4, 5) if mode == "fused" else (2, 3)}

        def move(kind):
            o, i = which[kind]
            for r in ranks:
                r.ctx.synchronize()  # every sender's pack kernel has finished
            recs = [r.buf[o].numel() // r.n_faces for r in ranks]
            assert len(set(recs)) == 1
            move_records(segments, [r.buf[o] for r in ranks], [r.buf[i] for r in ranks], recs[0])
            torch.cuda.synchronize()

        lockstep([(r.methods_points if mode == "methods" else r.fused_points)(n_steps) for r in ranks], move)
        out = []
        for r in ranks:
            r.ctx.synchronize()
            out.append((r.e.download(hfx.DISU_UPTS0), r.e.download(hfx.DIV_TCONF_UPTS)))
        grids = [hfx.fused_launch_grids(r.e.h) for r in ranks] if mode != "methods" else None
        return out, grids
    finally:
        for r in ranks:
            r.close()
