// Stand-alone driver of the interface-energy part of dfmdock_amd/csrc/dfm_poseprep.h for tests/test_ifenergy_cpu.py (built with the
// address and undefined-behaviour sanitizers, no GPU).  Reads one binary file - int32 Ar, Al; float32 cutoff, soft, elec_min_dist,
// dielectric_slope, center [3]; then per chain (receptor first) float32 xyz [n][3], rmin_half [n], sqrt_eps [n], charge [n] - runs the
// creator's checks in the creator's order and prints the first error, or the sum bound and the receptor's parameters in cell order.
#include <cstdio>
#include <cstdlib>

#include "dfm_poseprep.h"

struct Chain {
    std::vector<float> xyz, rh, se, q;
    bool read(FILE *f, int n)
    {
        const size_t m = (size_t)std::max(n, 0);
        xyz.resize(m * 3 + 1); rh.resize(m + 1); se.resize(m + 1); q.resize(m + 1);      // (never empty: an empty vector's data() may be NULL)
        return fread(xyz.data(), sizeof(float), m * 3, f) == m * 3 && fread(rh.data(), sizeof(float), m, f) == m &&
               fread(se.data(), sizeof(float), m, f) == m && fread(q.data(), sizeof(float), m, f) == m;
    }
};

static int fail(const std::string &msg, int rc)
{
    printf("error %s\n", msg.c_str());
    return rc;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 64;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 65;
    int32_t n[2];
    float sc[4], center[3];
    if (fread(n, sizeof(int32_t), 2, f) != 2 || fread(sc, sizeof(float), 4, f) != 4 || fread(center, sizeof(float), 3, f) != 3) return 66;
    Chain rec, lig;
    if (!rec.read(f, n[0]) || !lig.read(f, n[1])) return 66;
    fclose(f);
    std::string msg = dfm::check_atom_sets(n[0], rec.xyz.data(), n[1], lig.xyz.data(), center);
    if (msg.empty()) msg = dfm::check_iface_atoms("rec", n[0], rec.rh.data(), rec.se.data(), rec.q.data());
    if (msg.empty()) msg = dfm::check_iface_atoms("lig", n[1], lig.rh.data(), lig.se.data(), lig.q.data());
    if (msg.empty()) msg = dfm::check_iface_scalars(sc[0], sc[1], sc[2], sc[3]);
    if (!msg.empty()) return fail(msg, 2);
    dfm::CellGrid gr;
    if (!dfm::build_cell_grid(n[0], rec.xyz.data(), (double)sc[0], gr)) return fail("cells", 3);
    const dfm::IfaceBound b = dfm::iface_sum_bound(n[0], rec.se.data(), rec.q.data(), n[1], lig.se.data(), lig.q.data(), gr.max_cell, sc[1],
                                                   sc[2], sc[3]);
    printf("bound %.17g %.17g %.17g %d %d\n", b.term_kcal, b.pairs, b.sum_quanta, b.ok ? 1 : 0, gr.max_cell);
    if (n[0] <= 64) {
        const std::vector<float> par = dfm::gather_iface(gr.order, rec.rh.data(), rec.se.data(), rec.q.data());
        printf("rec_par");
        for (float v : par) printf(" %.9g", (double)v);
        printf("\norder");
        for (int32_t i : gr.order) printf(" %d", i);
        printf("\n");
    }
    return b.ok ? 0 : 4;
}
