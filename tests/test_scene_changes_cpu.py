"""What a scene's changes since its last commit make of the next commit (csrc/scene_changes.h), checked on the CPU against the rule it replaced.

The header is driven alone, by tests/sanitize/scene_changes_harness.cpp built with g++ and AddressSanitizer + UndefinedBehaviorSanitizer; nothing is loaded into Python.
The rule it replaced — three booleans in MRTScene_ written in seven places of api.cpp — is restated below as `Legacy`, writer by writer.  Every sequence of up to 6
events, on a flattened and on a two-level scene, from a fresh and from a committed scene, goes through both:

    V T O   the host changes vertices (mrt_scene_update_mesh), a transform (mrt_scene_set_instance_transform), something else (a mesh, a submesh, an option)
    D       vertices replaced on the device and not refitted there (mrt_scene_update_mesh_device / mrt_scene_update_blas_device); of a mesh no host change touches
    M       instances moved on the device (mrt_scene_set_instance_transforms_device), two-level scenes only
    S       a sync of the host copies (mrt_scene_sync_host_meshes: mrt_group_renderer_create on its template scene)
    C       mrt_scene_commit (which syncs first)

D and M happen only where the device entries are let in: on a committed scene (D: with the scene option refit).  At every commit
(a) the new recipe covers what changed, (b) where the old recipe covered it the new one is the same, (c) the sequences the old rule got wrong are the ones listed here.

The old rule's failures, minimal members (no single event can be left out), from a committed scene — all on two-level scenes, all ending in a TLAS-only commit
that leaves BLASes stale (first read from api.cpp as it was; tests/test_blas_device.py drives the four rows on the GPU, and run once against the library of the commit
before this header they failed there with wrong hits):

    M S V C        moved instances found by a sync, then mrt_scene_update_mesh (the one that needs no scene option refit)
    M S D C        moved instances found by a sync, an unrefitted mrt_scene_update_blas_device found later (here by the commit's own sync; M S D S C alike)
    D M S T C      both found by one sync, then mrt_scene_set_instance_transform (M D S T C alike: the two device entries commute)
    D M S M C      both found by one sync, then moved instances found again (M D S M C, D M S M S C alike)
"""
import os, shutil, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
SAN = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

MAX_EVENTS = 6
# what each recipe brings up to date.  't': transforms, 'v': vertices the host holds (its own, or a BLAS's read back), 'o': anything else,
# 'dv': vertices of a flattened scene that lie in the device's geometry buffers (g_pos / normals), where mrt_scene_update_mesh_device wrote them: build_keep_geometry
# flattens exactly those buffers, which is why the one exception to the join stands (scene_changes.h device_changes_found)
COVERS = {"T": {"t"}, "R": {"v"}, "F": {"v", "dv"}, "K": {"t", "dv"}, "B": {"t", "v", "dv", "o"}}


class Legacy:
    """MRTScene_::committed, only_vertices_changed, only_transforms_changed as api.cpp wrote them before scene_changes.h"""
    def __init__(self): self.c, self.oV, self.oT = False, False, False
    def copy(self): n = Legacy(); n.c, n.oV, n.oT = self.c, self.oV, self.oT; return n
    def mark_changed(self): self.c = self.oV = self.oT = False                      # mark_changed: a mesh, a submesh, an option
    def update_mesh(self):                                                          # mrt_scene_update_mesh
        if self.c: self.oV = True
        elif not self.oV: self.oT = False
        self.c = False
    def set_instance_transform(self):                                               # mrt_scene_set_instance_transform
        if self.c: self.oT = True
        if self.oV: self.oV = self.oT = False
        self.c = False
    def sync(self, flat, blas, moved):                                              # sync_host_meshes, its three branches in their order
        if flat and self.c: self.oV = True
        if blas:
            if self.c: self.oV = True
            elif self.oT: self.oV = self.oT = False
        if moved:
            if self.oV: self.oV = self.oT = False
            elif self.c: self.oT = True
    def commit(self, inst, refit, same):                                            # mrt_scene_commit: the recipe, then the flags
        if self.oT and inst and same: r = "T"
        elif self.oV and inst and refit: r = "R"                                    # (MRT_ERR_UNSUPPORTED from refit_two_level: build_scene(false, false) — the "else build" of the name)
        elif inst: r = "B"
        elif self.oT and self.oV: r = "both"                                        # build_scene(true, true): never reached (asserted below)
        elif self.oT: r = "K"
        elif self.oV and refit: r = "F"                                             # (build_scene ands its flag with the option)
        else: r = "B"
        self.oV = self.oT = False; self.c = True
        return r
    def says_pending(self): return (not self.c) and (self.oV or self.oT)            # device_entry_prologue's choice of words


def sequences(inst, refit, same, committed_start):
    """every sequence of up to MAX_EVENTS events that ends in a commit: (events, harness line, per token (committed, says pending, the old flags are sound), old recipe, changes at the commit)"""
    out = []
    def sound(L, known):          # do the two old flags say what the host knows to have changed?  (only transforms, device-side flattened vertices beside them or not; only vertices; neither)
        only_t = "t" in known and not known & {"v", "o"}
        only_v = bool(known) and known <= {"v", "dv"}
        return (L.oV, L.oT) == (only_v, only_t)
    def go(ev, line, toks, L, dv, dm, changes, known):
        if len(ev) == MAX_EVENTS: return
        for e in ("VTODMSC" if inst else "VTODSC"):
            L2, dv2, dm2, ch2, kn2, add = L.copy(), dv, dm, set(changes), set(known), "."
            if e == "V": L2.update_mesh(); ch2.add("v"); kn2.add("v"); add = "V"
            elif e == "T": L2.set_instance_transform(); ch2.add("t"); kn2.add("t"); add = "T"
            elif e == "O": L2.mark_changed(); ch2.add("o"); kn2.add("o"); add = "O"
            elif e == "D":
                if not (L.c and refit): continue
                dv2 = True; ch2.add("v" if inst else "dv")
            elif e == "M":
                if not L.c: continue
                dm2 = True; ch2.add("t")
            if e in "SC":
                mask = (1 if dv and not inst else 0) | (2 if dv and inst else 0) | (4 if dm else 0)
                L2.sync(bool(mask & 1), bool(mask & 2), bool(mask & 4)); dv2 = dm2 = False; add = str(mask)
                kn2 = set(ch2)
            toks2 = toks + [(L2.c, L2.says_pending(), sound(L2, kn2))]
            if e == "C":
                old = L2.commit(inst, refit, same); add += "C"; toks2 = toks2 + [(True, False, True)]
                out.append((ev + e, line + add, toks2, old, frozenset(ch2)))
                ch2, kn2 = set(), set()
            go(ev + e, line + add, toks2, L2, dv2, dm2, ch2, kn2)
    L = Legacy(); line = ""; toks = []
    if committed_start: L.commit(inst, refit, same); line = "0C"; toks = [(False, False, True), (True, False, True)]
    go("", line, toks, L, False, False, set(), set())
    return out


CONFIGS = [(inst, refit, same, start) for inst in (False, True) for refit in (False, True) for same in ((True, False) if inst else (True,)) for start in (False, True)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_changes") / "scene_changes_harness")
    p = subprocess.run(["g++", *SAN, "-o", exe, os.path.join(ROOT, "tests", "sanitize", "scene_changes_harness.cpp")], capture_output=True, text=True)
    if p.returncode != 0 and "sanitize" in p.stderr: pytest.skip("g++ without the sanitizer runtimes")
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def run_new(exe, cfg, seqs, planted=False):
    inst, refit, same, _ = cfg
    p = subprocess.run([exe, str(int(inst)), str(int(refit)), str(int(same))] + (["planted"] if planted else []), input="\n".join(s[1] for s in seqs) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-500:] + p.stderr[-2000:])
    lines = p.stdout.split("\n")[:len(seqs)]
    assert len(lines) == len(seqs)
    return [l.split() for l in lines]


def uncovered(seqs, tokens, which):
    """the sequences whose last commit's recipe (which: 'new' from the harness, 'old' from Legacy) leaves a change out"""
    bad = []
    for (ev, _, _, old, changes), tk in zip(seqs, tokens):
        r = tk[-1][2] if which == "new" else old
        if not changes <= COVERS.get(r, set()): bad.append(ev)
    return bad


@pytest.fixture(scope="module")
def enumerated(harness):
    res = {}
    for cfg in CONFIGS:
        seqs = sequences(*cfg)
        res[cfg] = (seqs, run_new(harness, cfg, seqs))
    return res


def test_harness_speaks_the_four_values_and_the_join(harness):
    cfg = (True, True, True, False)
    lines = ["", "0C", "0CV", "0CT", "0CVT", "0CTV", "0CO", "0CVV", "0CTT", "0C4", "0C2", "0C6", "0CT2", "O"]
    tk = run_new(harness, cfg, [(None, l) for l in lines])
    assert tk[0] == []                                            # (a scene starts as not committed, rebuild: the first token of the next line shows it after a sync that found nothing)
    assert tk[1] == ["0rB0", "1nB0"]
    assert [t[-1] for t in tk[2:]] == ["0vR1", "0tT1", "0rB0", "0rB0", "0rB0", "0vR1", "0tT1", "1tT0", "1vR0", "1rB0", "0rB0", "0rB0"]
    # device_entry_prologue's words: after a vertex change AND a transform change "scene not committed", as before (0CVT, 0CTV above end in ...0)
    flat = run_new(harness, (False, True, True, False), [(None, "0CT1"), (None, "0C1"), (None, "0CT"), (None, "0CV")])
    assert [t[-1] for t in flat] == ["0tK1", "1vF0", "0tK1", "0vF1"]          # the one exception: a flattened scene waiting with transforms keeps them when device-side vertices turn up


def test_committed_and_the_refusal_words_are_the_old_ones(enumerated):
    """`committed` is the old flag after every event.  device_entry_prologue chooses its words as the old flags did wherever those were sound, that is, wherever those said
    what the host knew to have changed; in the hole (the sequences of (c) and what follows them up to the next commit) the old words described a state that was not there"""
    for cfg, (seqs, tokens) in enumerated.items():
        for (ev, line, toks, _, _), tk in zip(seqs, tokens):
            assert [t[0] == "1" for t in tk] == [bool(c) for c, _, _ in toks], (cfg, ev, line, tk)
            assert all((t[3] == "1") == bool(p) for t, (_, p, ok) in zip(tk, toks) if ok), (cfg, ev, line, tk)


def test_a_new_recipe_covers_every_change(enumerated):
    n = 0
    for cfg, (seqs, tokens) in enumerated.items():
        assert uncovered(seqs, tokens, "new") == [], cfg
        n += len(seqs)
    assert n > 50000          # (what was enumerated: every sequence that ends in a commit, 12 configurations)


def test_where_the_old_recipe_was_right_the_new_one_is_the_same(enumerated):
    for cfg, (seqs, tokens) in enumerated.items():
        for (ev, _, _, old, changes), tk in zip(seqs, tokens):
            assert old != "both", (cfg, ev)
            if changes <= COVERS[old]: assert tk[-1][2] == old, (cfg, ev, old, tk[-1])


# (c) the old rule's failures: 1-minimal members per configuration (instancing, refit option, same instance list), from a committed scene
OLD_RULE_FAILS = {
    (True, True, True): {"MSVC", "MSDC", "DMSTC", "MDSTC", "DMSMC", "MDSMC"},
    (True, False, True): {"MSVC"},
    (True, True, False): {"MSVC", "MSDC"},          # (an instance list that is not the device's: the old rule falls through to refit_two_level, which answers MRT_ERR_UNSUPPORTED to such a scene and so ends in a build; by the table of recipes it is a miss all the same)
}
TABLE_ROWS = ["MSVC", "MSDSC", "DMSTC", "DMSMSC"]          # the issue's four rows, in this test's events


def is_subsequence(a, b):
    it = iter(b)
    return all(ch in it for ch in a)


def test_the_old_rule_fails_exactly_on_the_listed_sequences(enumerated):
    for cfg, (seqs, tokens) in enumerated.items():
        inst, refit, same, start = cfg
        fails = set(uncovered(seqs, tokens, "old"))
        # the failing commit alone matters: cut each sequence behind the last commit before it
        cut = {ev[ev[:-1].rfind("C") + 1:] for ev in fails}
        if not start:
            # a fresh scene meets them only behind its first commit; nothing fails before one
            assert all("C" in ev[:-1] for ev in fails), cfg
        minimal = {ev for ev in cut if not any((ev[:i] + ev[i + 1:]) in cut for i in range(len(ev) - 1))}
        if start:
            assert minimal == OLD_RULE_FAILS.get((inst, refit, same), set()), (cfg, sorted(minimal))
            for ev in cut: assert any(is_subsequence(m, ev) for m in minimal), (cfg, ev)
            if (inst, refit, same) == (True, True, True): assert all(r in fails for r in TABLE_ROWS)
        else:
            assert cut <= {ev[ev[:-1].rfind("C") + 1:] for ev in uncovered(*enumerated[(inst, refit, same, True)], "old")}, cfg          # (nothing a committed scene does not meet too)


def test_a_planted_join_that_forgets_the_transforms_is_caught(harness):
    """transforms + vertices = vertices: a vertex change and a transform change then refit and leave the instance rows stale; (a) must say so"""
    for cfg in ((True, True, True, True), (False, True, True, True)):
        seqs = sequences(*cfg)
        bad = uncovered(seqs, run_new(harness, cfg, seqs, planted=True), "new")
        assert "VTC" in bad and "TVC" in bad, cfg
