// Stand-alone driver of the hydrogen-bond part of dfmdock_amd/csrc/dfm_poseprep.h for tests/test_hbonds_cpu.py (built with the address
// and undefined-behaviour sanitizers, no GPU).  Reads one binary file - int32 Nr, Nl, n_rec_res, n_lig_res; float32 hb_cutoff,
// salt_cutoff; float64 min_cos2; float32 center [3]; int64 scratch budget in bytes; then per chain (receptor first) float32 xyz [n][3],
// float32 ante [n][3], uint8 role [n], int32 res [n] - runs the creator's checks in the creator's order and prints the first error, or
// what the creator would put on the device: both sorts, each atom's bits read back out of its float4's fourth component, the
// antecedents' x beside them, the charged residues and the chunk sizes.
#include <cstdio>
#include <cstdlib>

#include "dfm_poseprep.h"

struct Chain {
    std::vector<float> xyz, ante;
    std::vector<uint8_t> role;
    std::vector<int32_t> res;
    bool read(FILE *f, int n)
    {
        const size_t m = (size_t)std::max(n, 0);
        xyz.resize(m * 3 + 1); ante.resize(m * 3 + 1); role.resize(m + 1); res.resize(m + 1);      // (never empty: an empty vector's data() may be NULL)
        return fread(xyz.data(), sizeof(float), m * 3, f) == m * 3 && fread(ante.data(), sizeof(float), m * 3, f) == m * 3 &&
               fread(role.data(), 1, m, f) == m && fread(res.data(), sizeof(int32_t), m, f) == m;
    }
};

static int fail(const std::string &msg, int rc)
{
    printf("error %s\n", msg.c_str());
    return rc;
}

static void print_bits(const char *name, const std::vector<float> &v4)
{
    printf("%s", name);
    for (size_t q = 0; q < v4.size() / 4; ++q) {
        uint32_t b;
        std::memcpy(&b, &v4[q * 4 + 3], sizeof(b));
        printf(" %u", b);
    }
    printf("\n");
}

static void print_x(const char *name, const std::vector<float> &v4)
{
    printf("%s", name);
    for (size_t q = 0; q < v4.size() / 4; ++q) printf(" %.9g", (double)v4[q * 4]);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) return 64;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 65;
    int32_t n[4];
    float cut[2], center[3];
    double c2;
    int64_t budget;
    if (fread(n, sizeof(int32_t), 4, f) != 4 || fread(cut, sizeof(float), 2, f) != 2 || fread(&c2, sizeof(double), 1, f) != 1 ||
        fread(center, sizeof(float), 3, f) != 3 || fread(&budget, sizeof(int64_t), 1, f) != 1)
        return 66;
    Chain rec, lig;
    if (!rec.read(f, n[0]) || !lig.read(f, n[1])) return 66;
    fclose(f);
    std::string msg = dfm::check_atom_sets(n[0], rec.xyz.data(), n[1], lig.xyz.data(), center);
    if (msg.empty()) msg = dfm::check_hbond_chain("rec", n[0], rec.ante.data(), rec.role.data(), rec.res.data(), n[2]);
    if (msg.empty()) msg = dfm::check_hbond_chain("lig", n[1], lig.ante.data(), lig.role.data(), lig.res.data(), n[3]);
    if (msg.empty()) msg = dfm::check_hbond_scalars(cut[0], c2, cut[1]);
    if (!msg.empty()) return fail(msg, 2);
    const float reach = std::max(cut[0], cut[1]);
    dfm::CellGrid gr;
    if (!dfm::build_cell_grid(n[0], rec.xyz.data(), (double)reach, gr)) return fail("cells", 3);
    double llo[3] = {(double)lig.xyz[0], (double)lig.xyz[1], (double)lig.xyz[2]}, cen[3] = {(double)center[0], (double)center[1], (double)center[2]};
    for (int i = 1; i < n[1]; ++i)
        for (int k = 0; k < 3; ++k) llo[k] = std::min(llo[k], (double)lig.xyz[(size_t)i * 3 + k]);
    const dfm::LigandBlocks lb = dfm::build_ligand_blocks(n[1], lig.xyz.data(), llo, (double)reach, cen);
    std::vector<int32_t> rcomp, lcomp;
    const int Rc = dfm::hbond_charged_residues(n[0], rec.role.data(), rec.res.data(), n[2], rcomp);
    const int Lc = dfm::hbond_charged_residues(n[1], lig.role.data(), lig.res.data(), n[3], lcomp);
    printf("edge %.9g\norder", (double)reach);
    for (int32_t i : gr.order) printf(" %d", i);
    printf("\nlig_index");
    for (int32_t i : lb.index) printf(" %d", i);
    printf("\n");
    print_bits("rec_bits", dfm::gather4_hbond(gr.order, rec.xyz.data(), rec.role.data(), rec.res.data(), rcomp));
    print_bits("lig_bits", dfm::gather4_hbond(lb.index, lig.xyz.data(), lig.role.data(), lig.res.data(), lcomp));
    print_x("rec_x", dfm::gather4_hbond(gr.order, rec.xyz.data(), rec.role.data(), rec.res.data(), rcomp));
    print_x("rec_ante_x", dfm::gather4(gr.order, rec.ante.data(), nullptr));
    print_x("lig_ante_x", dfm::gather4(lb.index, lig.ante.data(), nullptr));
    printf("rec_compact");
    for (int32_t i : rcomp) printf(" %d", i);
    printf("\nlig_compact");
    for (int32_t i : lcomp) printf(" %d", i);
    printf("\ncharged %d %d\nwords %d\nchunk %d %d\n", Rc, Lc, dfm::rescon_words(Rc), dfm::hbond_chunk_poses(Lc, Rc),
           dfm::hbond_chunk_poses(Lc, Rc, (size_t)budget));
    return 0;
}
