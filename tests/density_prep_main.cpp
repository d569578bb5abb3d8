// Stand-alone driver of the density-fit part of dfmdock_amd/csrc/dfm_poseprep.h for tests/test_density_cpu.py (built with the address
// and undefined-behaviour sanitizers, no GPU).
//   density_prep bound Al            prints `bound <quanta> <ok>` of density_sum_bound
//   density_prep chunk Al per_atom   prints `chunk <poses>` of density_chunk_poses
//   density_prep FILE                reads int32 nx, ny, nz, C, Al, n_grid, n_atoms, n_w; float32 origin [3], voxel [3], center [3];
//                                    float32 grids [n_grid], lig_atoms [n_atoms], lig_w [n_w] (a count of 0: a NULL pointer); runs the
//                                    creator's checks in the creator's order and prints the first error, or the interleaved grid, the
//                                    atoms as the kernel reads them and the sum bound.
#include <cstdio>
#include <cstdlib>

#include "dfm_poseprep.h"

static int fail(const std::string &msg, int rc)
{
    printf("error %s\n", msg.c_str());
    return rc;
}

template <class T> static bool read_vec(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n + 1);      // (never empty: an empty vector's data() may be NULL)
    return fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc == 3 && std::string(argv[1]) == "bound") {
        const dfm::DensityBound b = dfm::density_sum_bound(atoll(argv[2]));
        printf("bound %.17g %d\n", b.quanta, b.ok ? 1 : 0);
        return 0;
    }
    if (argc == 4 && std::string(argv[1]) == "chunk") {
        printf("chunk %d\n", dfm::density_chunk_poses(atoi(argv[2]), atoi(argv[3]) != 0));
        return 0;
    }
    if (argc != 2) return 64;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 65;
    int32_t n[8];
    float geo[9];
    if (fread(n, sizeof(int32_t), 8, f) != 8 || fread(geo, sizeof(float), 9, f) != 9) return 66;
    const int nx = n[0], ny = n[1], nz = n[2], C = n[3], Al = n[4];
    std::vector<float> grids, atoms, w;
    if (!read_vec(f, grids, (size_t)n[5]) || !read_vec(f, atoms, (size_t)n[6]) || !read_vec(f, w, (size_t)n[7])) return 66;
    fclose(f);
    const float *g = n[5] ? grids.data() : nullptr, *a = n[6] ? atoms.data() : nullptr, *wp = n[7] ? w.data() : nullptr;
    std::string msg = dfm::check_density_grid(nx, ny, nz, geo, geo + 3, C, g);
    if (msg.empty()) msg = dfm::check_density_atoms(Al, a, wp, geo + 6);
    if (!msg.empty()) return fail(msg, 2);
    const dfm::DensityBound b = dfm::density_sum_bound(Al);
    printf("bound %.17g %d\n", b.quanta, b.ok ? 1 : 0);
    const std::vector<float> g4 = dfm::interleave_density(nx, ny, nz, C, g);
    printf("grid4");
    for (float v : g4) printf(" %a", (double)v);
    const std::vector<float> l4 = dfm::gather4_density(Al, a, wp);
    printf("\nlig4");
    for (float v : l4) printf(" %a", (double)v);
    printf("\n");
    return b.ok ? 0 : 4;
}
