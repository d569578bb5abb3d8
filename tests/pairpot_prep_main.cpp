// Stand-alone driver of the pair-potential part of dfmdock_amd/csrc/dfm_poseprep.h for tests/test_pairpot_cpu.py (built with the
// address and undefined-behaviour sanitizers, no GPU).
//   pairpot_prep bound Ar Al max_cell_atoms    prints `bound <pairs> <ok>` of pairpot_pair_bound
//   pairpot_prep chunk Al T NB per_atom counts prints `chunk <poses>` of pairpot_chunk_poses
//   pairpot_prep FILE                          reads int32 Ar, Al, T, NB, n_edges, n_table; float32 center [3]; per chain (receptor
//                                              first) float32 xyz [n][3], int32 type [n]; float32 edges [n_edges], table [n_table]
//                                              (n_edges / n_table = 0: a NULL pointer); runs the creator's checks in the creator's
//                                              order and prints the first error, or the quantised table in device order, the squared
//                                              edges, the receptor's second float4 in cell order and the pair bound.
#include <cinttypes>
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
    if (argc == 5 && std::string(argv[1]) == "bound") {
        const dfm::PairpotBound b = dfm::pairpot_pair_bound(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
        printf("bound %.17g %d\n", b.pairs, b.ok ? 1 : 0);
        return 0;
    }
    if (argc == 7 && std::string(argv[1]) == "chunk") {
        printf("chunk %d\n", dfm::pairpot_chunk_poses(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]) != 0, atoi(argv[6]) != 0));
        return 0;
    }
    if (argc != 2) return 64;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 65;
    int32_t n[6];
    float center[3];
    if (fread(n, sizeof(int32_t), 6, f) != 6 || fread(center, sizeof(float), 3, f) != 3) return 66;
    const int Ar = n[0], Al = n[1], T = n[2], NB = n[3];
    std::vector<float> rec, lig, edges, table;
    std::vector<int32_t> rt, lt;
    if (!read_vec(f, rec, (size_t)std::max(Ar, 0) * 3) || !read_vec(f, rt, (size_t)std::max(Ar, 0))) return 66;
    if (!read_vec(f, lig, (size_t)std::max(Al, 0) * 3) || !read_vec(f, lt, (size_t)std::max(Al, 0))) return 66;
    if (!read_vec(f, edges, (size_t)n[4]) || !read_vec(f, table, (size_t)n[5])) return 66;
    fclose(f);
    const float *e = n[4] ? edges.data() : nullptr, *tb = n[5] ? table.data() : nullptr;
    std::string msg = dfm::check_atom_sets(Ar, rec.data(), Al, lig.data(), center);
    if (msg.empty() && (T < 1 || T > dfm::PAIRPOT_MAX_TYPES)) msg = "need 1 <= T <= " + std::to_string(dfm::PAIRPOT_MAX_TYPES);
    if (msg.empty()) msg = dfm::check_pairpot_edges(NB, e);
    if (msg.empty()) msg = dfm::check_pairpot_table(T, NB, tb);
    if (msg.empty()) msg = dfm::check_pairpot_types("rec", Ar, rt.data(), T);
    if (msg.empty()) msg = dfm::check_pairpot_types("lig", Al, lt.data(), T);
    if (!msg.empty()) return fail(msg, 2);
    dfm::PoseFrame fr;
    msg = dfm::build_pose_frame(Ar, rec.data(), Al, lig.data(), center, e[NB], "last edge", fr);
    if (!msg.empty()) return fail(msg, 3);
    const dfm::PairpotBound b = dfm::pairpot_pair_bound(Ar, Al, fr.gr.max_cell);
    printf("bound %.17g %d %d\n", b.pairs, b.ok ? 1 : 0, fr.gr.max_cell);
    const std::vector<int32_t> q = dfm::quantise_pairpot(T, NB, tb);
    printf("table_q");
    for (int32_t v : q) printf(" %" PRId32, v);
    const std::vector<double> e2 = dfm::pairpot_edges2(NB, e);
    printf("\ne2");
    for (double v : e2) printf(" %a", v);
    const std::vector<float> par = dfm::gather4_pairpot(fr.gr.order, rt.data(), T, NB);
    printf("\nrec_par");
    for (size_t i = 0; i < par.size(); ++i) {
        int32_t bits;
        std::memcpy(&bits, &par[i], sizeof(bits));
        printf(" %" PRId32, bits);
    }
    printf("\norder");
    for (int32_t i : fr.gr.order) printf(" %d", i);
    printf("\nthr %a\n", (double)fr.thr);
    return b.ok ? 0 : 4;
}
