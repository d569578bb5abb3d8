// Stand-alone driver of build_pose_frame (dfmdock_amd/csrc/dfm_poseprep.h) for tests/test_pose_prep_cpu.py (built with the address and
// undefined-behaviour sanitizers, no GPU).  argv: a binary file - int32 Ar, Al; float32 reach; float32 center [3], rec [Ar][3],
// lig [Al][3] - and the reach's name.  Prints the frame as text: doubles with 17, floats with 9 significant digits; a refusal as
// "error <message>".
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
    if (argc != 3) return 64;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 65;
    int32_t n[2];
    float reach, center[3];
    if (fread(n, sizeof(int32_t), 2, f) != 2 || fread(&reach, sizeof(float), 1, f) != 1 || fread(center, sizeof(float), 3, f) != 3) return 66;
    const size_t nr = (size_t)std::max(n[0], 0) * 3, nl = (size_t)std::max(n[1], 0) * 3;
    std::vector<float> rec(nr ? nr : 1), lig(nl ? nl : 1);      // (never empty: an empty vector's data() may be NULL)
    if (fread(rec.data(), sizeof(float), nr, f) != nr || fread(lig.data(), sizeof(float), nl, f) != nl) return 66;
    fclose(f);
    std::string msg = dfm::check_atom_sets(n[0], rec.data(), n[1], lig.data(), center);
    if (!msg.empty()) {
        printf("error %s\n", msg.c_str());
        return 2;
    }
    dfm::PoseFrame fr;
    msg = dfm::build_pose_frame(n[0], rec.data(), n[1], lig.data(), center, reach, argv[2], fr);
    auto d = [](double x) { printf(" %.17g", x); };
    auto g = [](float x) { printf(" %.9g", (double)x); };
    auto i = [](int x) { printf(" %d", x); };
    if (!msg.empty()) {
        printf("error %s\n", msg.c_str());
        if (!fr.lb.sphere.empty()) row("finite", std::vector<int>{fr.lb.finite ? 1 : 0}, i);
        return 3;
    }
    const dfm::WalkGrid &w = fr.g;
    row("lo", w.lo, d);
    row("hi", w.hi, d);
    row("center", w.center, d);
    row("dims", std::vector<int>{w.nx, w.ny, w.nz, fr.gr.max_cell}, i);
    row("edge_grow", std::vector<double>{w.edge, w.grow}, d);
    row("thr_reject2", std::vector<float>{fr.thr, fr.reject2}, g);
    row("cell_start", fr.gr.start, i);
    row("order", fr.gr.order, i);
    row("lig_lo", fr.lig_lo, d);
    row("lig_index", fr.lb.index, i);
    row("sphere", fr.lb.sphere, g);
    row("finite", std::vector<int>{fr.lb.finite ? 1 : 0}, i);
    return 0;
}
