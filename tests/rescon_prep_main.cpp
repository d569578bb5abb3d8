// Stand-alone driver of the residue-contact part of dfmdock_amd/csrc/dfm_poseprep.h for tests/test_affinity_cpu.py (built with the
// address and undefined-behaviour sanitizers, no GPU).  Reads one binary file - int32 Ar, Al, Rr, Lr; float32 cutoff, center [3]; int64
// scratch budget in bytes; then per chain (receptor first) float32 xyz [n][3], int32 res [n], uint8 class [n_res] - runs the creator's
// checks in the creator's order and prints the first error, or what the creator would put on the device: both chains' residue indices
// in their sorted order (read back out of the float4's fourth component), the class masks, the row words and the chunk sizes.
#include <cstdio>
#include <cstdlib>

#include "dfm_poseprep.h"

struct Chain {
    std::vector<float> xyz;
    std::vector<int32_t> res;
    std::vector<uint8_t> cls;
    bool read(FILE *f, int n, int n_res)
    {
        const size_t m = (size_t)std::max(n, 0), r = (size_t)std::min(std::max(n_res, 0), 1 << 16);
        xyz.resize(m * 3 + 1); res.resize(m + 1); cls.resize(r + 1);      // (never empty: an empty vector's data() may be NULL)
        return fread(xyz.data(), sizeof(float), m * 3, f) == m * 3 && fread(res.data(), sizeof(int32_t), m, f) == m &&
               fread(cls.data(), 1, r, f) == r;
    }
};

static int fail(const std::string &msg, int rc)
{
    printf("error %s\n", msg.c_str());
    return rc;
}

static void print_w(const char *name, const std::vector<float> &v4)
{
    printf("%s", name);
    for (size_t q = 0; q < v4.size() / 4; ++q) {
        int32_t r;
        std::memcpy(&r, &v4[q * 4 + 3], sizeof(r));
        printf(" %d", r);
    }
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) return 64;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 65;
    int32_t n[4];
    float cutoff, center[3];
    int64_t budget;
    if (fread(n, sizeof(int32_t), 4, f) != 4 || fread(&cutoff, sizeof(float), 1, f) != 1 || fread(center, sizeof(float), 3, f) != 3 ||
        fread(&budget, sizeof(int64_t), 1, f) != 1)
        return 66;
    Chain rec, lig;
    if (!rec.read(f, n[0], n[2]) || !lig.read(f, n[1], n[3])) return 66;
    fclose(f);
    std::string msg = dfm::check_atom_sets(n[0], rec.xyz.data(), n[1], lig.xyz.data(), center);
    if (msg.empty()) msg = dfm::check_rescon_chain("rec", n[0], rec.res.data(), n[2], rec.cls.data());
    if (msg.empty()) msg = dfm::check_rescon_chain("lig", n[1], lig.res.data(), n[3], lig.cls.data());
    if (msg.empty()) msg = dfm::check_rescon_cutoff(cutoff);
    if (!msg.empty()) return fail(msg, 2);
    dfm::CellGrid gr;
    if (!dfm::build_cell_grid(n[0], rec.xyz.data(), (double)cutoff, gr)) return fail("cells", 3);
    double llo[3] = {(double)lig.xyz[0], (double)lig.xyz[1], (double)lig.xyz[2]}, cen[3] = {(double)center[0], (double)center[1], (double)center[2]};
    for (int i = 1; i < n[1]; ++i)
        for (int k = 0; k < 3; ++k) llo[k] = std::min(llo[k], (double)lig.xyz[(size_t)i * 3 + k]);
    const dfm::LigandBlocks lb = dfm::build_ligand_blocks(n[1], lig.xyz.data(), llo, (double)cutoff, cen);
    const std::vector<float> rec4 = dfm::gather4_res(gr.order, rec.xyz.data(), rec.res.data());
    const std::vector<float> lig4 = dfm::gather4_res(lb.index, lig.xyz.data(), lig.res.data());
    printf("order");
    for (int32_t i : gr.order) printf(" %d", i);
    printf("\nlig_index");
    for (int32_t i : lb.index) printf(" %d", i);
    printf("\n");
    print_w("rec_res", rec4);
    print_w("lig_res", lig4);
    printf("rec_x");
    for (size_t q = 0; q < rec4.size() / 4; ++q) printf(" %.9g", (double)rec4[q * 4]);
    printf("\nmasks");
    for (uint32_t v : dfm::rescon_class_masks(n[2], rec.cls.data())) printf(" %u", v);
    printf("\nwords %d\nchunk %d %d\n", dfm::rescon_words(n[2]), dfm::rescon_chunk_poses(n[3], n[2]), dfm::rescon_chunk_poses(n[3], n[2], (size_t)budget));
    return 0;
}
