"""Exact audit of a committed rope layout (scene_device.h "traversal node"), in numpy: the 64-byte binary nodes with eight escape links each that
traverse.h and traverse_instanced.h walk — the query entries, every BLAS of a two-level scene, scenes without the 8-wide layout, and the renderer's
rope = 1 / wide = 0 walks.  Boxes are float32 values and links are integers, so everything is compared exactly; the one bound is bvh_audit's 1e-12
relative clip bound for pre-split references.  (bvh_audit.py is the same audit of the 8-wide layout; what both need is imported from it.)

    lay = layout_of(device_scene)          # DeviceScene.read_layout("header" / "rope_nodes" / "rope_packets" / "instances")
    rep = audit(lay, presplit=False, num_tris=T)     # bvh_audit.Report: .failures (strings naming tree, node, octant or axis, packet), .counts
    rep.check()                            # AssertionError listing the failures
    links_kept(before, after).check()      # a refit wrote nothing but boxes and packet vertices

Trees.  A flattened scene has one tree rooted at node 0 over all of "rope_nodes" / "rope_packets".  A two-level scene has one tree per BLAS: its
instances' rows name its first node (node_base, the root), its first packet (packet_base) and its packet count (ntri); its nodes end where the next
BLAS's begin.  Inside a BLAS every child index, every escape link and every leaf's first packet is RELATIVE to those bases (two_level.hip copies
each BLAS's nodes and packets as they were built, and traverse_instanced.h adds node_base / packet_base to every index it follows); NODE_TERM stays
what it is.  Node and packet numbers in the failures are absolute positions in the two parts.

Checks (names as they start a failure):
  structure   every index inside its tree's arrays; every node reached exactly once from the root through a / b & NODE_INDEX_MASK (walked level by
              level, every node expanded at most once: a cycle is a failure, not a hang); the leaves' [first, first + count) ranges partition the
              tree's packets, count >= 1; every triangle id referenced — exactly once unless the scene was built with pre-splitting, and exactly
              0 .. ntri - 1 in a BLAS; the BLASes' node sets disjoint and covering the part; instances of one BLAS name one root.
  escape      esc[o](root) = NODE_TERM, and for an internal node p whose near child for octant o is the right one when bit o of its mask is set:
              esc[o](near) = far, esc[o](far) = esc[o](p) — what traverse.h relies on (on a hit it enters near, on a miss it follows esc).  Checked
              node against parent, which is the rule applied to all eight words of every node, with a wrong word reported where it is.
  union       an internal node's lo / hi are the float32 min / max of its two children's, bit for bit (k_refit of the build and k_rope_refit both
              compute exactly that; min / max of floats is exact and associative).  The one freedom: where the children's values are equal as numbers
              and differ in bits (-0 against +0) either child's bits are accepted, since fminf / fmaxf may return either.
  contain     every packet's exact triangle (float64 sums of the stored float32 words) inside its leaf's box, for unsplit references.
  pad         ... with at least half of k_flatten's pad (1e-5 |coord| + 1e-6) to spare.  Excused: the packets whose triangle id occurs in more than
              one packet (pre-split references: k_split_emit pads the clipped piece) and no other; counts["pad_excused"] says how many, and it is a
              failure for it not to be zero when the scene was built without pre-splitting.
  split       pre-split references by the clipped piece (bvh_audit.check_split) against their leaf boxes; the ancestors follow from union.
  links_kept  between two read-backs of one tree: words 3, 7 and 8 .. 15 of every node and the id word of every packet unchanged."""
import numpy as np

from bvh_audit import Report, check_split, decode_instances, decode_packets, pad_of, ulp_of

NODE_LEAF, NODE_TERM, NODE_INDEX_MASK = 0x80000000, 0xFFFFFFFF, 0x00FFFFFF


def layout_of(ds):
    """the rope layout of a committed DeviceScene and what names its trees"""
    hdr = ds.read_layout("header")
    lay = dict(header=hdr, rope_nodes=ds.read_layout("rope_nodes"), rope_packets=ds.read_layout("rope_packets"))
    if hdr[2]:
        lay["instances"] = ds.read_layout("instances")
    return lay


def trees_of(lay):
    """[(name, root, node_end, packet_base, packet_count)] — one flattened tree, or one entry per BLAS with triangles (in order of node_base)"""
    N, P = len(lay["rope_nodes"]), len(lay["rope_packets"])
    if not int(np.asarray(lay["header"])[2]):
        return [("tree 0", 0, N, 0, P)] if N else []
    inst = decode_instances(lay["instances"])
    seen = {}
    for i in range(len(inst["blas"])):
        if inst["ntri"][i] > 0:
            seen.setdefault(int(inst["blas"][i]), (int(inst["node_base"][i]), int(inst["packet_base"][i]), int(inst["ntri"][i])))
    order = sorted(seen.items(), key=lambda kv: kv[1][0])
    out = []
    for k, (b, (nb, pb, nt)) in enumerate(order):
        end = order[k + 1][1][0] if k + 1 < len(order) else N
        out.append((f"BLAS {b}", nb, end, pb, nt))
    return out


def _walk(rep, name, a, b, leaf, root, end, seen, parent):
    """Level by level from root; node indices absolute, children = base + stored index (base = root).  Every node is expanded at most once, so the walk
    ends after at most end - root expansions whatever the links say.  Returns the levels (arrays of nodes reached for the first time, root first)."""
    levels = []
    front = np.array([root], np.int64)
    while len(front):
        uniq, cnt = np.unique(front, return_counts=True)
        first = seen[uniq] == 0
        seen[uniq] += cnt
        for nd in uniq[seen[uniq] > 1][:10]:
            rep.fail(f"structure: {name} node {nd}: reached {seen[nd]} times (parent {parent[nd]}): a shared child or a cycle")
        new = uniq[first]
        levels.append(new)
        inner = new[~leaf[new]]
        kids = np.concatenate([root + a[inner], root + (b[inner] & NODE_INDEX_MASK)])
        par = np.concatenate([inner, inner])
        ok = (kids >= root) & (kids < end)
        for p, c in list(zip(par[~ok], kids[~ok]))[:10]:
            rep.fail(f"structure: {name} node {p}: child index {c - root} outside the tree's {end - root} nodes")
        kids, par = kids[ok], par[ok]
        parent[kids] = par
        front = kids
    return levels


def audit(lay, presplit=False, num_tris=None, check_pad=True):
    """Audit the rope layout of one scene (layout_of).  presplit: the flattened scene was built with pre-splitting allowed (BLASes never are).
    num_tris: triangles of a flattened scene (every id 0 .. num_tris - 1 must be referenced)."""
    rep = Report()
    wn = np.ascontiguousarray(lay["rope_nodes"], np.uint32).reshape(-1, 16)
    wp = np.ascontiguousarray(lay["rope_packets"], np.uint32).reshape(-1, 12)
    N, P = len(wn), len(wp)
    two = bool(int(np.asarray(lay["header"])[2]))
    rep.counts.update(nodes=N, leaves=0, packets=P, trees=0, pad_excused=0)
    if N == 0:
        rep.fail("structure: no rope layout"); return rep
    lo32, hi32 = wn[:, 0:3].view(np.float32), wn[:, 4:7].view(np.float32)
    lo, hi = lo32.astype(np.float64), hi32.astype(np.float64)
    a, b = wn[:, 3].astype(np.int64), wn[:, 7].astype(np.int64)
    esc = wn[:, 8:16].astype(np.int64)
    leaf = (a & NODE_LEAF) != 0
    V, gid = decode_packets(wp)
    trees = trees_of(lay)
    rep.counts["trees"] = len(trees)
    if two:
        inst = decode_instances(lay["instances"])
        for bl in np.unique(inst["blas"][inst["ntri"] > 0]):
            rows = np.nonzero((inst["blas"] == bl) & (inst["ntri"] > 0))[0]
            for f in ("node_base", "packet_base", "ntri"):
                if len(np.unique(inst[f][rows])) > 1:
                    rep.fail(f"structure: BLAS {bl}: its instances {rows.tolist()} name different {f}: {inst[f][rows].tolist()}")
    seen = np.zeros(N, np.int64)
    parent = np.full(N, -1, np.int64)
    owner = np.full(N, -1, np.int64)
    pk_leaf = np.full(P, -1, np.int64)
    split_any = np.zeros(P, bool)
    for t, (name, root, end, pb, nt) in enumerate(trees):
        if not (0 <= root < end <= N):
            rep.fail(f"structure: {name}: nodes {root} .. {end - 1} outside the part's {N}"); continue
        if not (0 <= pb and pb + nt <= P):
            rep.fail(f"structure: {name}: packets {pb} .. {pb + nt - 1} outside the part's {P}"); continue
        levels = _walk(rep, name, a, b, leaf, root, end, seen, parent)
        mine = np.concatenate(levels)          # (a node another tree reached before is a failure of the walk and is not expanded again)
        owner[mine] = t
        for nd in (np.nonzero(seen[root:end] == 0)[0] + root)[:10]:
            rep.fail(f"structure: {name} node {nd}: never reached from the root {root}")
        # ---- leaves: ranges partition the tree's packets
        lv = mine[leaf[mine]]
        rep.counts["leaves"] += int(len(lv))
        first, cnt = a[lv] & 0x7FFFFFFF, b[lv]
        bad = (cnt < 1) | (first + cnt > nt)
        for nd, f_, c_ in list(zip(lv[bad], first[bad], cnt[bad]))[:10]:
            rep.fail(f"structure: {name} node {nd}: leaf range first {f_} count {c_} outside the tree's {nt} packets" if c_ >= 1 else f"structure: {name} node {nd}: leaf with count {c_}")
        lv, first, cnt = lv[~bad], first[~bad], cnt[~bad]
        cover = np.zeros(nt + 1, np.int64)
        np.add.at(cover, first, 1); np.add.at(cover, first + cnt, -1)
        cover = np.cumsum(cover)[:nt]
        ids = np.repeat(lv, cnt)                                        # per referenced packet, in leaf order: its leaf
        pos = np.repeat(first - np.cumsum(cnt) + cnt, cnt) + np.arange(int(cnt.sum()))
        for j in np.nonzero(cover != 1)[0][:10]:
            who = lv[(first <= j) & (j < first + cnt)] if cover[j] else lv[first + cnt == j]
            rep.fail(f"structure: {name} packet {pb + j} (id {gid[pb + j]}): referenced by {cover[j]} leaves"
                     + (" (" + ", ".join(f"node {w}" for w in who) + (")" if cover[j] else " ends just before it)") if len(who) else ""))
        pk_leaf[pb + pos] = ids                                        # (a packet in two ranges: the last one; already a failure)
        # ---- triangle ids
        g = gid[pb:pb + nt]
        n_t = nt if two else int(num_tris) if num_tris is not None else (int(g.max()) + 1 if nt else 0)
        if ((g < 0) | (g >= n_t)).any():
            j = int(np.nonzero((g < 0) | (g >= n_t))[0][0])
            rep.fail(f"structure: {name} packet {pb + j}: id {g[j]} outside 0 .. {n_t - 1}")
        gc = np.bincount(g[(g >= 0) & (g < n_t)], minlength=n_t)
        for m in np.nonzero(gc == 0)[0][:10]:
            rep.fail(f"structure: {name}: triangle {m} referenced by no packet")
        multi = gc > 1
        if two or not presplit:
            for m in np.nonzero(multi)[0][:10]:
                rep.fail(f"structure: {name}: triangle {m} referenced by {gc[m]} packets with pre-splitting off (packets {(np.nonzero(g == m)[0] + pb).tolist()})")
        inside = (g >= 0) & (g < n_t)
        split_any[pb:pb + nt][inside] = multi[g[inside]]
        # ---- escape links: node against parent
        rel = lambda x: np.where(x == NODE_TERM, -1, root + x)          # stored link -> absolute node (-1: the walk is over)
        for o in range(8):
            if esc[root, o] != NODE_TERM:
                rep.fail(f"escape: {name} node {root} octant {o}: the root's link is {esc[root, o]}, not NODE_TERM")
        inner = mine[~leaf[mine]]
        la, rb = root + a[inner], root + (b[inner] & NODE_INDEX_MASK)
        okc = (la >= root) & (la < end) & (rb >= root) & (rb < end)
        inner, la, rb = inner[okc], la[okc], rb[okc]
        for o in range(8):
            right_first = ((b[inner] >> (24 + o)) & 1) != 0
            near, far = np.where(right_first, rb, la), np.where(right_first, la, rb)
            got_n, got_f, up = rel(esc[near, o]), rel(esc[far, o]), rel(esc[inner, o])
            for k in np.nonzero(got_n != far)[0][:6]:
                rep.fail(f"escape: {name} node {near[k]} octant {o}: link {got_n[k]} but it is the near child of node {inner[k]} (mask bit {int(right_first[k])}), whose far child is {far[k]}")
            for k in np.nonzero(got_f != up)[0][:6]:
                rep.fail(f"escape: {name} node {far[k]} octant {o}: link {got_f[k]} but it is the far child of node {inner[k]} (mask bit {int(right_first[k])}), whose own link is {up[k]}")
        # ---- union: parent box = min / max of the children's, bit for bit (either child's bits where the two are equal as numbers)
        for side, box32, fn in (("lo", lo32, np.minimum), ("hi", hi32, np.maximum)):
            want = fn(box32[la], box32[rb])
            pbit, lbit, rbit = box32[inner].view(np.uint32), box32[la].view(np.uint32), box32[rb].view(np.uint32)
            good = (box32[inner] == want) & ((pbit == lbit) | (pbit == rbit))
            for k, ax in list(zip(*np.nonzero(~good)))[:10]:
                rep.fail(f"union: {name} node {inner[k]} axis {'xyz'[ax]} {side}: {box32[inner[k], ax]!r} is not the {fn.__name__} of its children's "
                         f"{box32[la[k], ax]!r} (node {la[k]}) and {box32[rb[k], ax]!r} (node {rb[k]})")
    if two:
        for nd in np.nonzero(owner < 0)[0][:10]:
            rep.fail(f"structure: node {nd}: in no BLAS's tree")
    # ---- contain / pad: every unsplit packet against its leaf's box
    rep.counts["pad_excused"] = int(split_any.sum())
    if (two or not presplit) and split_any.any():
        rep.fail(f"pad: {int(split_any.sum())} packets excused from the pad check in a scene built without pre-splitting")
    tlo, thi = V.min(1), V.max(1)
    m = np.maximum(np.abs(tlo), np.abs(thi))
    pad, ulp = pad_of(m), ulp_of(m)
    sel = np.nonzero((pk_leaf >= 0) & ~split_any)[0]
    if len(sel):
        nd = pk_leaf[sel]
        mlo, mhi = tlo[sel] - lo[nd], hi[nd] - thi[sel]
        mg = np.minimum(mlo, mhi)
        frac = np.stack([mlo, mhi], -1) / pad[sel][..., None]
        bad = (mg < 0).any(1)
        for k in np.nonzero(bad)[0][:20]:
            ax = int(np.argmin(mg[k])); side = "lo" if mlo[k, ax] < mhi[k, ax] else "hi"
            rep.fail(f"contain: packet {sel[k]} (id {gid[sel[k]]}) outside its leaf node {nd[k]} axis {'xyz'[ax]} {side} by {-mg[k, ax]:.3e} ({-mg[k, ax] / ulp[sel[k], ax]:.2f} ulp)")
        fr = frac.reshape(len(sel), 6)
        amin = np.argmin(fr, 1); fmin = fr[np.arange(len(sel)), amin]
        k = int(np.argmin(fmin)); ax, s = divmod(int(amin[k]), 2)
        mv = (mlo if s == 0 else mhi)[k, ax]
        rep.note("contain", mv, mv / ulp[sel[k], ax], fmin[k], f"packet {sel[k]} node {nd[k]} axis {'xyz'[ax]} {'lo' if s == 0 else 'hi'}")
        rep.margins["pad"] = dict(rep.margins["contain"])
        if check_pad:
            for k in np.nonzero((fmin < 0.5) & ~bad)[0][:20]:
                ax, s = divmod(int(amin[k]), 2)
                rep.fail(f"pad: packet {sel[k]} (id {gid[sel[k]]}) in leaf node {nd[k]} axis {'xyz'[ax]} {'lo' if s == 0 else 'hi'}: margin {fmin[k]:.3f} of the pad {pad[sel[k], ax]:.3e}")
    # ---- pre-split references: the clipped piece against the leaf boxes
    refs_all = np.nonzero(split_any & (pk_leaf >= 0))[0]
    if len(refs_all):
        order = refs_all[np.argsort(gid[refs_all], kind="stable")]
        ids, start = np.unique(gid[order], return_index=True)
        for g, b0, b1 in zip(ids, start, np.r_[start[1:], len(order)]):
            refs = order[b0:b1]
            nd = pk_leaf[refs]
            check_split(rep, g, refs, V[refs[0]], lo[nd], hi[nd], lambda j: ((int(nd[j]), lo[nd[j]], hi[nd[j]]),), lambda tag: f"leaf node {tag}")
    return rep


def links_kept(before, after):
    """what a refit must leave alone, between two layout_of read-backs of one tree: a / b (words 3 and 7: leaf ranges, child indices, near masks), the
    eight escape links (words 8 .. 15) and every packet's id word"""
    rep = Report()
    n0, n1 = np.asarray(before["rope_nodes"], np.uint32), np.asarray(after["rope_nodes"], np.uint32)
    p0, p1 = np.asarray(before["rope_packets"], np.uint32), np.asarray(after["rope_packets"], np.uint32)
    if n0.shape != n1.shape or p0.shape != p1.shape:
        rep.fail(f"links_kept: {n0.shape[0]} nodes and {p0.shape[0]} packets before, {n1.shape[0]} and {p1.shape[0]} after"); return rep
    words = [3, 7] + list(range(8, 16))
    for nd, k in list(zip(*np.nonzero(n0[:, words] != n1[:, words])))[:20]:
        w = words[k]
        rep.fail(f"links_kept: node {nd} word {w}" + (f" (octant {w - 8})" if w >= 8 else "") + f": {n0[nd, w]:#x} before, {n1[nd, w]:#x} after")
    for j in np.nonzero(p0[:, 3] != p1[:, 3])[0][:20]:
        rep.fail(f"links_kept: packet {j}: id {p0[j, 3]} before, {p1[j, 3]} after")
    rep.counts.update(nodes=int(len(n0)), packets=int(len(p0)))
    return rep
