// scene_changes_harness.cpp — drives csrc/scene_changes.h alone (tests/test_scene_changes_cpu.py).
// usage: scene_changes_harness <instancing 0|1> <refit option 0|1> <same instance list 0|1> [planted]   < sequences
// One sequence of events per input line, every sequence on a scene of its own:
//   V T O   the host changed vertices / a transform / something else (a mesh, a submesh, an option)
//   0 .. 7  a sync of the host copies found: bit 0 flattened vertices, bit 1 BLAS vertices, bit 2 moved instances
//   C       mrt_scene_commit succeeded (its own sync is the digit in front of it)
//   .       nothing that touches the value (a device entry)
// One token per event on the output line: committed 0/1, pending n/t/v/r, the recipe a commit takes now (for C: the one it took) T/R/K/F/B, and whether a refused
// device entry would say "host-side changes are pending" 0/1.
// `planted` swaps the join for one with transforms + vertices = vertices: the test's check (a) has to catch it.
#include "scene_changes.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using mrt::Pending;
static constexpr Pending planted_join(Pending a, Pending b) {
    if ((a == Pending::transforms && b == Pending::vertices) || (a == Pending::vertices && b == Pending::transforms)) return Pending::vertices;
    return mrt::join(a, b);
}

template <class Changes> static int run(bool instancing, bool refit, bool same_list) {
    static char line[4096], out[5 * 4096];
    while (fgets(line, sizeof line, stdin)) {
        Changes s;
        size_t o = 0;
        for (const char *p = line; *p && *p != '\n'; p++) {
            mrt::CommitRecipe r = s.recipe(instancing, refit, same_list);
            switch (*p) {
            case 'V': s.host_changed(Pending::vertices); break;
            case 'T': s.host_changed(Pending::transforms); break;
            case 'O': s.host_changed(Pending::rebuild); break;
            case 'C': s.commit_done(); break;
            case '.': break;
            default:
                if (*p < '0' || *p > '7') { fprintf(stderr, "unknown event '%c'\n", *p); return 2; }
                s.device_changes_found((*p - '0') & 1, (*p - '0') & 2, (*p - '0') & 4);
            }
            if (*p != 'C') r = s.recipe(instancing, refit, same_list);
            out[o++] = s.committed() ? '1' : '0';
            out[o++] = "ntvr"[(int)s.pending()];
            out[o++] = "TRKFB"[(int)r];
            out[o++] = s.host_changes_pending() ? '1' : '0';
            out[o++] = ' ';
        }
        out[o] = 0;
        puts(out);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s instancing refit same_list [planted]\n", argv[0]); return 2; }
    const bool a = atoi(argv[1]) != 0, b = atoi(argv[2]) != 0, c = atoi(argv[3]) != 0;
    if (argc > 4 && !strcmp(argv[4], "planted")) return run<mrt::SceneChangesOver<planted_join>>(a, b, c);
    return run<mrt::SceneChanges>(a, b, c);
}
