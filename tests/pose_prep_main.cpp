// Stand-alone driver of dfmdock_amd/csrc/dfm_poseprep.h for tests/test_pose_prep_cpu.py (built with the address and undefined-behaviour
// sanitizers, no GPU).  Reads one binary file - int32 Ar, Al; float64 edge; float32 center [3], rec [Ar][3], lig [Al][3] - and prints the
// receptor's cell grid, the ligand's own grid origin and the ligand blocks as text: doubles with 17, floats with 9 significant digits.
#include <cstdio>
#include <cstdlib>

#include "dfm_poseprep.h"

template <class V, class P>
static void row(const char *name, const V &v, P print)
{
    printf("%s", name);
    for (const auto &x : v) print(x);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) return 64;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 65;
    int32_t n[2];
    double edge;
    float center[3];
    if (fread(n, sizeof(int32_t), 2, f) != 2 || fread(&edge, sizeof(double), 1, f) != 1 || fread(center, sizeof(float), 3, f) != 3) return 66;
    const size_t nr = (size_t)std::max(n[0], 0) * 3, nl = (size_t)std::max(n[1], 0) * 3;
    std::vector<float> rec(nr ? nr : 1), lig(nl ? nl : 1);      // (never empty: an empty vector's data() may be NULL)
    if (fread(rec.data(), sizeof(float), nr, f) != nr || fread(lig.data(), sizeof(float), nl, f) != nl) return 66;
    fclose(f);
    const std::string msg = dfm::check_atom_sets(n[0], rec.data(), n[1], lig.data(), center);
    if (!msg.empty()) {
        printf("error %s\n", msg.c_str());
        return 2;
    }
    dfm::CellGrid gr, gl;
    if (!dfm::build_cell_grid(n[0], rec.data(), edge, gr) || !dfm::build_cell_grid(n[1], lig.data(), edge, gl)) {
        printf("error cells\n");
        return 3;
    }
    const dfm::WalkGrid w = dfm::walk_grid(gr, edge, edge, center);
    const dfm::LigandBlocks lb = dfm::build_ligand_blocks(n[1], lig.data(), gl.lo, edge, w.center);
    auto d = [](double x) { printf(" %.17g", x); };
    auto g = [](float x) { printf(" %.9g", (double)x); };
    auto i = [](int x) { printf(" %d", x); };
    row("lo", w.lo, d);
    row("hi", w.hi, d);
    row("dims", std::vector<int>{w.nx, w.ny, w.nz, gr.max_cell}, i);
    row("cell_start", gr.start, i);
    row("order", gr.order, i);
    row("lig_lo", gl.lo, d);
    row("lig_index", lb.index, i);
    row("sphere", lb.sphere, g);
    row("finite", std::vector<int>{lb.finite ? 1 : 0}, i);
    row("slack", std::vector<float>{dfm::pose_slack(w.hi[0]), dfm::pose_slack(1e5)}, g);
    return 0;
}
