"""Exact audit of a committed 8-wide layout (scene_device.h "wide node"), in numpy float64.

Every plane of a node is p + q * 2^e: a float32 origin plus an 8-bit multiple of a power of two, which float64 holds exactly.  The audit decodes
every slot, walks the trees from their roots and checks that every box the builder, the quantiser, the refit and the TLAS build emitted encloses
what the triangle test can accept: the triangle {v0, v0 + e1, v0 + e2} of every packet, summed exactly from the stored float32 words.

    lay = layout_of(device_scene)          # DeviceScene.read_layout of every part
    rep = audit(lay, presplit=False)       # Report: .failures (strings naming node, slot, axis, packet), .margins (smallest margin per check)
    rep.check()                            # AssertionError listing the failures

Checks (names as in Report.margins):
  structure   every node reached exactly once from node 0 and the instances' BLAS roots; every index inside its array; real depth <= stats.wide_depth
              (two-level: TLAS levels + 1 + the deepest BLAS); every triangle id referenced, exactly once when nothing was pre-split.
  contain     zero-margin containment of every packet's exact triangle in its leaf slot and in every ancestor slot.
  pad         the leaf padding survives quantisation: every such plane lies beyond the triangle's extreme by at least half of k_flatten's pad
              1e-5 |coord| + 1e-6 (bvh_build.hip: the quantiser only rounds outwards from the padded box, traverse_wide.h relies on the pad).
  split       pre-split references (one triangle in several packets): their slot boxes, ordered along the split axis, cover the triangle's extent there
              without a gap, and the triangle clipped to each reference's share of that axis lies inside its box (float64 clip, 1e-12 relative).
              Their planes are checked for containment only: k_split_emit pads the clipped piece, not the triangle.
  tlas_leaf   each instance's 8-wide TLAS leaf slot (and every ancestor slot) contains its padded world box from inst_box.
  obj_box     the object-space part of inst_box contains every triangle of the BLAS with half a pad to spare.  (It is the BLAS's root box, the union
              of the padded leaf boxes; the decoded root SLOTS may reach up to a grid step beyond it, which is harmless, so they are not compared.)
  world_box   the world box contains the exact image, under M' (the float64 inverse of the stored float32 w2o rows), of the object box grown by the
              rounding bound of the device's fma chain: delta_k = gamma_4 (sum_j |R_kj| max|X_j| + |w_k|), X over the world box.
Margins are reported in float32 ulps of the coordinate and as a fraction of the pad.

Which layout: this audit covers the 8-wide layout only (wnodes / wpackets, the 8-wide TLAS slots, inst_box).  The rope layout — the 64-byte binary nodes
with escape links of a flattened scene built with rope = 1 or wide = 0, and of every BLAS — is audited by rope_audit.py, which imports Report, pad_of,
the packet decoding and check_split from here; the rope TLAS's links are checked by tlas_resort_reference.py.
"""
import numpy as np

U = 2.0 ** -24
GAMMA4 = 4 * U / (1 - 4 * U)
EMPTY_LO, EMPTY_HI = 255, 0


# ------------------------------------------------------------------------------------------------ decoding
def _bytes(words):
    """(..., k) uint32 -> (..., 4k) uint8, little-endian byte order of the device"""
    return np.ascontiguousarray(words, np.uint32).view(np.uint8).reshape(words.shape[:-1] + (4 * words.shape[-1],))


def decode_nodes(wn):
    """wn: (N, 20) uint32.  Returns a dict of float64 slot boxes lo/hi (N, 8, 3), qlo/qhi (N, 8, 3) bytes, imask (N,), child_base, tri_base,
    meta (N, 8) bytes, exponents (N, 3), origin (N, 3)."""
    wn = np.ascontiguousarray(wn, np.uint32).reshape(-1, 20)
    n = wn.shape[0]
    origin = wn[:, 0:3].view(np.float32).astype(np.float64)
    ew = wn[:, 3]
    ex = np.stack([((ew >> (8 * a)) & 0xFF).astype(np.uint8).view(np.int8).astype(np.int64) for a in range(3)], 1)
    imask = (ew >> 24).astype(np.uint32)
    q = _bytes(wn[:, 8:20]).reshape(n, 6, 8)            # qlo_x qlo_y qlo_z qhi_x qhi_y qhi_z, 8 slots each
    qlo = np.transpose(q[:, 0:3, :], (0, 2, 1)).astype(np.int64)
    qhi = np.transpose(q[:, 3:6, :], (0, 2, 1)).astype(np.int64)
    step = np.ldexp(1.0, ex)[:, None, :]
    lo = origin[:, None, :] + qlo * step
    hi = origin[:, None, :] + qhi * step
    meta = _bytes(wn[:, 6:8]).reshape(n, 8).astype(np.int64)
    return dict(n=n, origin=origin, ex=ex, imask=imask, child_base=wn[:, 4].astype(np.int64), tri_base=wn[:, 5].astype(np.int64),
                meta=meta, qlo=qlo, qhi=qhi, lo=lo, hi=hi)


def decode_packets(wp):
    """wp: (P, 4 x stride) uint32 -> v (P, 3, 3) float64 exact vertices, gid (P,)"""
    wp = np.ascontiguousarray(wp, np.uint32)
    f = wp[:, :12].view(np.float32).astype(np.float64).reshape(-1, 3, 4)
    v0 = f[:, 0, :3]
    v = np.stack([v0, v0 + f[:, 1, :3], v0 + f[:, 2, :3]], 1)
    return v, wp[:, 3].astype(np.int64)


def decode_instances(rows):
    """rows: (I, 20) uint32 InstanceDev -> w2o (I, 3, 4) float64, and the index fields"""
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, 20)
    w2o = rows[:, 0:12].view(np.float32).astype(np.float64).reshape(-1, 3, 4)
    f = {k: rows[:, 12 + i].astype(np.int64) for i, k in enumerate(("node_base", "packet_base", "gid_base", "ts_base", "vbase", "ntri", "blas", "wroot"))}
    f["w2o"] = w2o
    return f


def layout_of(ds):
    """every part of a committed DeviceScene's 8-wide layout (DeviceScene.read_layout)"""
    hdr = ds.read_layout("header")
    lay = dict(header=hdr, wnodes=ds.read_layout("wnodes"), wpackets=ds.read_layout("wpackets"))
    if hdr[2]:
        lay.update(instances=ds.read_layout("instances"), inst_box=ds.read_layout("inst_box"), wtlas_index=ds.read_layout("wtlas_index"))
    return lay


def pad_of(m):
    """k_flatten's pad of a coordinate range whose largest magnitude is m (float32 arithmetic, as on the device)"""
    m = np.asarray(m, np.float32)
    return (np.float32(1e-5) * m + np.float32(1e-6)).astype(np.float64)


def ulp_of(m):
    return np.spacing(np.abs(np.asarray(m, np.float64)).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ report
class Report:
    def __init__(self):
        self.failures = []
        self.margins = {}        # check -> dict(min_abs, min_ulp, min_pad_frac, where)
        self.counts = {}
        self.depth = None
        self.thin = None         # per packet: smallest margin in pads, and (axis, side) of that plane (the probes aim there)

    def fail(self, msg):
        if len(self.failures) < 200:
            self.failures.append(msg)

    def note(self, check, margin, ulps, frac, where):
        cur = self.margins.get(check)
        if cur is None or frac < cur["min_pad_frac"] or (frac == cur["min_pad_frac"] and margin < cur["min_abs"]):
            self.margins[check] = dict(min_abs=float(margin), min_ulp=float(ulps), min_pad_frac=float(frac), where=where)

    def check(self):
        assert not self.failures, f"{len(self.failures)} audit failure(s):\n" + "\n".join(self.failures[:40])

    def summary(self):
        return {k: (round(v["min_ulp"], 2), round(v["min_pad_frac"], 4)) for k, v in self.margins.items()}


# ------------------------------------------------------------------------------------------------ the walk
def _walk(D, roots, rep, npk, tlas_entries, tlas_nodes=None):
    """Depth-first from each root.  Returns parent[node] = (node, slot) of the slot that names it (-1 for roots), depth per root, and the leaf
    references: list of (node, slot, first, count) — packet ranges, or wtlas_index ranges in the TLAS slots [0, tlas_nodes)."""
    N = D["n"]
    seen = np.zeros(N, np.int64)
    parent = np.full((N, 2), -1, np.int64)
    leaves = []
    depths = {}
    for root in roots:
        if not (0 <= root < N):
            rep.fail(f"root {root} outside wnodes ({N})"); continue
        stack = [(root, 1)]
        dmax = 0
        while stack:
            nd, d = stack.pop()
            seen[nd] += 1
            if seen[nd] > 1:
                rep.fail(f"node {nd}: reached {seen[nd]} times"); continue
            dmax = max(dmax, d)
            im = int(D["imask"][nd]); cb = int(D["child_base"][nd]); tb = int(D["tri_base"][nd])
            rank = 0
            for sl in range(8):
                m = int(D["meta"][nd, sl]); cnt, off = m >> 5, m & 31
                internal = (im >> sl) & 1
                empty = (D["qlo"][nd, sl] == EMPTY_LO).all() and (D["qhi"][nd, sl] == EMPTY_HI).all()
                if empty:
                    if internal or cnt:
                        rep.fail(f"node {nd} slot {sl}: empty box (qlo = 255, qhi = 0) but imask bit {internal}, meta count {cnt}")
                    continue
                if internal and cnt:
                    rep.fail(f"node {nd} slot {sl}: both an internal and a leaf child")
                if internal:
                    c = cb + rank; rank += 1
                    if not (0 <= c < N):
                        rep.fail(f"node {nd} slot {sl}: child index {c} outside wnodes ({N})"); continue
                    if c <= nd:
                        rep.fail(f"node {nd} slot {sl}: child {c} does not come after its parent"); continue
                    if tlas_nodes is not None and (nd < tlas_nodes) != (c < tlas_nodes):
                        rep.fail(f"node {nd} slot {sl}: child {c} crosses between the TLAS slots and the BLASes"); continue
                    parent[c] = (nd, sl)
                    stack.append((c, d + 1))
                elif cnt:
                    if off + cnt > 32:
                        rep.fail(f"node {nd} slot {sl}: leaf range {off}+{cnt} beyond the 32-bit mask")
                    lim = npk if (tlas_nodes is None or nd >= tlas_nodes) else tlas_entries
                    if tb + off + cnt > lim:
                        rep.fail(f"node {nd} slot {sl}: leaf range {tb + off}..{tb + off + cnt - 1} outside its array ({lim})"); continue
                    leaves.append((nd, sl, tb + off, cnt))
                else:
                    rep.fail(f"node {nd} slot {sl}: a box with neither a child node nor packets")
        depths[root] = dmax
    return seen, parent, leaves, depths


def _chain_boxes(D, parent, node, slot):
    """the decoded boxes of (node, slot) and of every ancestor slot: list of (node, slot, lo, hi)"""
    out = []
    while node >= 0:
        out.append((node, slot, D["lo"][node, slot], D["hi"][node, slot]))
        node, slot = parent[node]
    return out


def _clip_extent(v, axis, a, b):
    """float64 extent (lo3, hi3) of triangle v (3, 3) clipped to a <= x[axis] <= b; None if empty"""
    poly = [np.asarray(p, np.float64) for p in v]
    for bound, keep_ge in ((a, True), (b, False)):
        out = []
        for i in range(len(poly)):
            p, q = poly[i], poly[(i + 1) % len(poly)]
            pin = p[axis] >= bound if keep_ge else p[axis] <= bound
            qin = q[axis] >= bound if keep_ge else q[axis] <= bound
            if pin:
                out.append(p)
            if pin != qin:
                t = (bound - p[axis]) / (q[axis] - p[axis])
                r = p + (q - p) * t; r[axis] = bound
                out.append(r)
        poly = out
        if not poly:
            return None
    P = np.array(poly)
    return P.min(0), P.max(0)


def check_split(rep, g, refs, v, lo, hi, chain, name):
    """One pre-split triangle g (exact vertices v) whose references are the packets refs with the leaf boxes lo / hi (one row per reference): ordered along
    some axis the boxes cover the triangle's extent there without a gap, and the triangle clipped to each reference's share of that axis lies inside every
    box of chain(j) — (tag, lo, hi) of reference j's leaf box and whatever encloses it — within 1e-12 relative.  name(tag) words a box for the messages.
    Shared by the audits of both layouts (the 8-wide one here, the rope one in rope_audit.py)."""
    tl_, th_ = v.min(0), v.max(0)
    scale = max(1.0, float(np.abs(v).max()))
    tol = 1e-12 * scale
    best = None
    for ax in range(3):
        o = np.argsort(lo[:, ax], kind="stable")
        L, H = lo[o, ax], hi[o, ax]
        if L[0] > tl_[ax] + tol or H.max() < th_[ax] - tol:
            continue
        cuts = [tl_[ax]]
        ok = True
        for k in range(len(o) - 1):
            reach = H[:k + 1].max()
            if reach < L[k + 1] - tol and reach < th_[ax]:
                ok = False; break
            cuts.append(min(max(0.5 * (min(H[k], reach) + L[k + 1]), cuts[-1]), th_[ax]))
        cuts.append(th_[ax])
        if not ok:
            continue
        worst, where = np.inf, None
        for k, j in enumerate(o):
            a, b = cuts[k], cuts[k + 1]
            if b < a:
                continue
            ext = _clip_extent(v, ax, a, b)
            if ext is None:
                continue
            r = refs[j]
            for tag, blo, bhi in chain(j):
                mm = np.minimum(ext[0] - blo, bhi - ext[1])
                mm[ax] = min(a - blo[ax], bhi[ax] - b)
                if mm.min() < worst:
                    worst, where = float(mm.min()), (r, tag, int(np.argmin(mm)))
        if best is None or worst > best[0]:
            best = (worst, where, ax)
    if best is None:
        rep.fail(f"split: triangle {g}: its {len(refs)} references leave a gap along every axis"); return
    worst, where, ax = best
    if worst < -tol:
        r, tag, a = where
        rep.fail(f"split: triangle {g} clipped to reference packet {r}'s share of axis {'xyz'[ax]} leaves {name(tag)} on axis {'xyz'[a]} by {-worst:.3e}")
    elif where is not None:
        a = where[2]
        rep.note("split", worst, worst / ulp_of(scale), worst / pad_of(scale), f"triangle {g} packet {where[0]} {name(where[1])} axis {'xyz'[a]}")


def audit(lay, presplit=False, num_tris=None, check_pad=True):
    """Audit one layout (layout_of).  presplit: the scene was built with pre-splitting allowed (flattened scenes only; BLASes never are).
    num_tris: triangles of a flattened scene (every id 0 .. num_tris - 1 must be referenced)."""
    rep = Report()
    hdr = np.asarray(lay["header"], np.int64)
    NW, tlas_wcap, I, wide_depth = int(hdr[0]), int(hdr[1]), int(hdr[2]), int(hdr[3])
    if NW == 0:
        rep.fail("no 8-wide layout"); return rep
    D = decode_nodes(lay["wnodes"])
    if D["n"] != NW:
        rep.fail(f"header says {NW} nodes, {D['n']} read")
    V, gid = decode_packets(lay["wpackets"])
    P = V.shape[0]
    two = I > 0
    if two:
        inst = decode_instances(lay["instances"])
        ibox = np.asarray(lay["inst_box"], np.float32).astype(np.float64).reshape(-1, 4, 4)[:, :, :3]
        wtl = np.asarray(lay["wtlas_index"], np.int64)
        blas_roots = sorted(set(int(r) for r in inst["wroot"][inst["ntri"] > 0]))
        roots = [0] + blas_roots
    else:
        roots = [0]
    seen, parent, leaves, depths = _walk(D, roots, rep, P, len(wtl) if two else P, tlas_nodes=tlas_wcap if two else None)
    # ---- structure: reachability, depth, ids
    unreached = np.nonzero(seen[tlas_wcap if two else 0:] == 0)[0] + (tlas_wcap if two else 0)
    for nd in unreached[:10]:
        rep.fail(f"node {nd}: never reached from a root")
    if two:
        real = depths.get(0, 0) + 1 + max([depths.get(r, 0) for r in blas_roots] or [0])
    else:
        real = depths.get(0, 0)
    rep.depth = real
    if real > wide_depth:
        rep.fail(f"real depth {real} exceeds the claimed wide_depth {wide_depth}" + (f" (TLAS {depths.get(0, 0)} + 1 + deepest BLAS)" if two else ""))
    pk_leaf = np.full((P, 2), -1, np.int64)
    tl_leaf = {}
    for nd, sl, first, cnt in leaves:
        if two and nd < tlas_wcap:
            for j in range(first, first + cnt):
                ins = int(wtl[j])
                if not (0 <= ins < I):
                    rep.fail(f"TLAS node {nd} slot {sl}: instance id {ins} out of range"); continue
                if ins in tl_leaf:
                    rep.fail(f"instance {ins}: in two TLAS leaf slots")
                tl_leaf[ins] = (nd, sl)
            continue
        for j in range(first, first + cnt):
            if pk_leaf[j, 0] >= 0:
                rep.fail(f"packet {j}: referenced by node {pk_leaf[j, 0]} slot {pk_leaf[j, 1]} and by node {nd} slot {sl}")
            pk_leaf[j] = (nd, sl)
    for j in np.nonzero(pk_leaf[:, 0] < 0)[0][:10]:
        rep.fail(f"packet {j} (id {gid[j]}): referenced by no leaf slot")
    rep.counts["packets"] = int(P); rep.counts["nodes_reached"] = int((seen > 0).sum())
    if two:
        for i in range(I):
            if inst["ntri"][i] > 0 and i not in tl_leaf:
                rep.fail(f"instance {i}: in no TLAS leaf slot")
        blas_seen = {}
        for i in range(I):
            b = int(inst["blas"][i])
            if b in blas_seen or inst["ntri"][i] == 0:
                continue
            pb, nt = int(inst["packet_base"][i]), int(inst["ntri"][i])
            blas_seen[b] = (pb, nt, i)
            if pb + nt > P:
                rep.fail(f"instance {i}: packets {pb}..{pb + nt - 1} outside wpackets ({P})"); continue
            ids = np.sort(gid[pb:pb + nt])
            if not np.array_equal(ids, np.arange(nt)):
                rep.fail(f"BLAS {b} (instance {i}): packet ids are not exactly 0 .. {nt - 1} once each")
        split_ids = np.zeros(0, np.int64)
    else:
        n_t = int(num_tris) if num_tris is not None else int(gid.max()) + 1 if P else 0
        cnt = np.bincount(gid, minlength=n_t) if P else np.zeros(n_t, np.int64)
        if (gid >= n_t).any() or (gid < 0).any():
            rep.fail(f"packet ids outside 0 .. {n_t - 1}")
        missing = np.nonzero(cnt[:n_t] == 0)[0]
        for g in missing[:10]:
            rep.fail(f"triangle {g}: referenced by no packet")
        multi = np.nonzero(cnt > 1)[0]
        if not presplit:
            for g in multi[:10]:
                rep.fail(f"triangle {g}: referenced {cnt[g]} times with pre-splitting off")
            split_ids = np.zeros(0, np.int64)
        else:
            split_ids = multi
        rep.counts["split_triangles"] = int(len(split_ids))
    # ---- containment and pad, packet by packet up the chain (vectorised over packets, one level per step)
    is_split = np.isin(gid, split_ids) if (not two and len(split_ids)) else np.zeros(P, bool)
    tlo, thi = V.min(1), V.max(1)
    m = np.maximum(np.abs(tlo), np.abs(thi))
    pad = pad_of(m)
    ulp = ulp_of(m)
    thin = np.full(P, np.inf); thin_ax = np.zeros((P, 2), np.int64)
    sel = np.nonzero((pk_leaf[:, 0] >= 0) & ~is_split)[0]
    node, slot = pk_leaf[sel, 0].copy(), pk_leaf[sel, 1].copy()
    level = 0
    while len(sel):
        blo, bhi = D["lo"][node, slot], D["hi"][node, slot]
        mlo, mhi = tlo[sel] - blo, bhi - thi[sel]              # >= 0: contained; >= pad / 2: the padding survived
        mg = np.minimum(mlo, mhi)
        frac = np.stack([mlo, mhi], -1) / pad[sel][..., None]  # (n, 3, 2)
        bad = (mg < 0).any(1)
        for k in np.nonzero(bad)[0][:20]:
            a = int(np.argmin(mg[k])); side = "lo" if mlo[k, a] < mhi[k, a] else "hi"
            rep.fail(f"contain: packet {sel[k]} (id {gid[sel[k]]}) outside node {node[k]} slot {slot[k]} axis {'xyz'[a]} {side} by {-mg[k, a]:.3e} "
                     f"({-mg[k, a] / ulp[sel[k], a]:.2f} ulp){' (leaf slot)' if level == 0 else ''}")
        fr = frac.reshape(len(sel), 6)
        amin = np.argmin(fr, 1); fmin = fr[np.arange(len(sel)), amin]
        better = fmin < thin[sel]
        thin[sel[better]] = fmin[better]; thin_ax[sel[better]] = np.c_[amin[better] // 2, amin[better] % 2]
        if len(sel):
            k = int(np.argmin(fmin)); a, s = divmod(int(amin[k]), 2)
            mv = (mlo if s == 0 else mhi)[k, a]
            rep.note("contain", mv, mv / ulp[sel[k], a], fmin[k], f"packet {sel[k]} node {node[k]} slot {slot[k]} axis {'xyz'[a]} {'lo' if s == 0 else 'hi'}")
            if check_pad:
                low = np.nonzero((fmin < 0.5) & ~bad)[0]
                for k in low[:20]:
                    a, s = divmod(int(amin[k]), 2)
                    rep.fail(f"pad: packet {sel[k]} (id {gid[sel[k]]}) in node {node[k]} slot {slot[k]} axis {'xyz'[a]} {'lo' if s == 0 else 'hi'}: "
                             f"margin {fmin[k]:.3f} of the pad {pad[sel[k], a]:.3e}")
        nxt = parent[node]
        keep = nxt[:, 0] >= 0
        sel, node, slot = sel[keep], nxt[keep, 0], nxt[keep, 1]
        level += 1
    rep.thin = (thin, thin_ax)
    if "contain" in rep.margins:
        rep.margins["pad"] = dict(rep.margins["contain"])
    # ---- pre-split references
    if len(split_ids):
        order = np.argsort(gid, kind="stable")
        bounds = np.searchsorted(gid[order], split_ids), np.searchsorted(gid[order], split_ids, side="right")
        for g, b0, b1 in zip(split_ids, *bounds):
            refs = order[b0:b1]
            refs = refs[pk_leaf[refs, 0] >= 0]
            lo = np.array([D["lo"][pk_leaf[r, 0], pk_leaf[r, 1]] for r in refs]); hi = np.array([D["hi"][pk_leaf[r, 0], pk_leaf[r, 1]] for r in refs])
            check_split(rep, g, refs, V[refs[0]], lo, hi, lambda j: (((nd, sl), blo, bhi) for nd, sl, blo, bhi in _chain_boxes(D, parent, pk_leaf[refs[j], 0], pk_leaf[refs[j], 1])),
                        lambda tag: f"node {tag[0]} slot {tag[1]}")
    # ---- TLAS
    if two:
        for i, (nd, sl) in tl_leaf.items():
            wlo, whi = ibox[i, 2], ibox[i, 3]
            for n2, s2, blo, bhi in _chain_boxes(D, parent, nd, sl):
                mg = np.minimum(wlo - blo, bhi - whi)
                wm = np.maximum(np.abs(wlo), np.abs(whi))
                a = int(np.argmin(mg))
                if mg[a] < 0:
                    rep.fail(f"tlas_leaf: instance {i} world box outside TLAS node {n2} slot {s2} axis {'xyz'[a]} by {-mg[a]:.3e}")
                rep.note("tlas_leaf", mg[a], mg[a] / ulp_of(wm[a]), mg[a] / pad_of(wm[a]), f"instance {i} node {n2} slot {s2} axis {'xyz'[a]}")
        for b, (pb, nt, i0) in blas_seen.items():
            olo, ohi = ibox[i0, 0], ibox[i0, 1]
            for i in range(I):
                if inst["blas"][i] == b and inst["ntri"][i] > 0 and not (np.array_equal(ibox[i, 0], olo) and np.array_equal(ibox[i, 1], ohi)):
                    rep.fail(f"obj_box: instances {i0} and {i} of BLAS {b} carry different object boxes")
            if pb + nt > P:
                continue
            mlo, mhi = tlo[pb:pb + nt] - olo, ohi - thi[pb:pb + nt]
            frac = np.minimum(mlo, mhi) / pad[pb:pb + nt]
            k, a = np.unravel_index(int(np.argmin(frac)), frac.shape)
            mg = min(mlo[k, a], mhi[k, a])
            if mg < 0:
                rep.fail(f"obj_box: BLAS {b} packet {pb + k} outside the object box of inst_box axis {'xyz'[a]} by {-mg:.3e}")
            elif check_pad and frac[k, a] < 0.5:
                rep.fail(f"obj_box: BLAS {b} packet {pb + k} axis {'xyz'[a]}: margin {frac[k, a]:.3f} of the pad")
            rep.note("obj_box", mg, mg / ulp[pb + k, a], frac[k, a], f"BLAS {b} packet {pb + k} axis {'xyz'[a]}")
        for i in range(I):
            if inst["ntri"][i] == 0:
                continue
            R = inst["w2o"][i]
            A, w = R[:, :3], R[:, 3]
            try:
                M = np.linalg.inv(A)
            except np.linalg.LinAlgError:
                rep.fail(f"world_box: instance {i}: singular w2o rows"); continue
            wlo, whi = ibox[i, 2], ibox[i, 3]
            X = np.maximum(np.abs(wlo), np.abs(whi))
            delta = GAMMA4 * (np.abs(A) @ X + np.abs(w))
            olo, ohi = ibox[i, 0] - delta, ibox[i, 1] + delta
            corners = np.array([[(ohi if (c >> k) & 1 else olo)[k] for k in range(3)] for c in range(8)])
            img = (corners - w) @ M.T                               # x = A^-1 (p - w)
            mlo, mhi = img.min(0) - wlo, whi - img.max(0)
            mg = np.minimum(mlo, mhi); a = int(np.argmin(mg))
            wm = X[a]
            if mg[a] < 0:
                rep.fail(f"world_box: instance {i}: the image of its object box grown by delta = {delta.max():.3e} leaves the world box on axis {'xyz'[a]} "
                         f"{'lo' if mlo[a] < mhi[a] else 'hi'} by {-mg[a]:.3e} (pad {pad_of(wm):.3e})")
            rep.note("world_box", mg[a], mg[a] / ulp_of(wm), mg[a] / pad_of(wm), f"instance {i} axis {'xyz'[a]}")
    return rep


def thinnest(rep, lay, k):
    """the k packets with the smallest pad margin: (packet, axis, side) with side 0 = lo plane, 1 = hi plane"""
    thin, ax = rep.thin
    fin = np.nonzero(np.isfinite(thin))[0]
    o = fin[np.argsort(thin[fin], kind="stable")[:k]]
    return o, ax[o, 0], ax[o, 1]
