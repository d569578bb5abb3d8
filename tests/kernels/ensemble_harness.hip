// ensemble_harness.hip - test-only host shim around the clustering and consensus launchers of libdfmdock_amd.so
// (tests/ensemble_harness.py builds it): dfm::launch_pose_dist, launch_cluster_leader, launch_cluster_count, launch_cluster_step,
// launch_contact_bits, launch_contact_count, launch_contact_score.
//
// Host code only: no kernels here.  The guard-band protocol is harness_common.h's.  BEFORE anything is uploaded this file checks that
// every array is large enough for the launch it feeds, that order is a permutation of 0..B-1 and pos its inverse, that res lies in
// [0, L) without repeats, that 1 <= B <= 65536 and max_clusters >= 1, that the step's U and state name nothing outside their arrays,
// and that outputs are flagged as outputs (a failure is hipErrorInvalidValue and no device is touched).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../dfmdock_amd/csrc/dfm_internal.h"
#include "harness_common.h"

namespace {

// buffer slots of one call (tests/ensemble_harness.py SLOTS lists the same names in the same order)
enum Slot {
    S_X, S_RES, S_RMSD, S_MASK, S_ORDER, S_POS, S_COUNTS, S_U, S_CLUSTER_OF, S_CENTER, S_SIZE, S_N_OUT, S_MLIST, S_STATE,
    S_REC, S_LIG, S_BITS, S_MEMBER, S_COUNT, S_REC_COUNT, S_LIG_COUNT, S_N_CONTACTS, S_SCORE_SUM,
    N_SLOTS
};

enum Op { OP_POSE_RMSD, OP_POSE_MASK, OP_LEADER, OP_COUNT, OP_STEP, OP_SIZE_FULL, OP_CONTACT_BITS, OP_CONTACT_COUNT, OP_CONTACT_SCORE, OP_CONSENSUS_FULL };

constexpr long long MAX_CONSENSUS = 4096;      // poses and residues of one consensus launch of this shim

}  // namespace

extern "C" {

struct Call {
    harness::HarnessBuf buf[N_SLOTS];
    float radius, cutoff;
    // B poses of L ligand residues, n_res of them compared (res unused: n_res = L); n poses of a consensus chunk, R receptor residues
    int B, L, n_res, max_clusters, n, R;
};

HARNESS_EXPORTS(Call)

int kh_run(const Call *c, int op)
{
    const long long B = c->B, L = c->L, n = c->n, R = c->R;
    auto has = [&](int i, long long bytes) { return c->buf[i].host && c->buf[i].bytes >= bytes; };
    auto in = [&](int i, long long bytes) { return has(i, bytes) && c->buf[i].out == 0; };
    auto out = [&](int i, long long bytes) { return has(i, bytes) && c->buf[i].out == 1; };      // sentinel interior
    auto io = [&](int i, long long bytes) { return has(i, bytes) && c->buf[i].out == 2; };       // the host's interior uploaded first
    auto interior = [&](int i) { return (const char *)c->buf[i].host + (c->buf[i].out ? harness::GUARD : 0); };
    bool ok = true;
    const long long W32 = (B + 31) / 32, W64 = (L + 63) / 64;
    const long long maxc = c->max_clusters < B ? c->max_clusters : B;

    if (op == OP_POSE_RMSD || op == OP_POSE_MASK) {
        ok = B >= 1 && B <= dfm::CL_MAX_POSES && L >= 1 && L <= 65536 && c->n_res >= 1 && c->n_res <= L && in(S_X, B * L * 36);
        if (ok && c->buf[S_RES].host) {
            ok = in(S_RES, (long long)c->n_res * 4);
            if (ok) {
                const int32_t *r = (const int32_t *)c->buf[S_RES].host;
                std::vector<char> seen((size_t)L, 0);
                for (int k = 0; k < c->n_res && ok; ++k) {
                    ok = r[k] >= 0 && r[k] < L && !seen[(size_t)r[k]];
                    if (ok) seen[(size_t)r[k]] = 1;
                }
            }
        } else if (ok) {
            ok = c->n_res == L;
        }
        ok = ok && (op == OP_POSE_RMSD ? out(S_RMSD, B * B * 4) : out(S_MASK, B * W32 * 4) && c->radius > 0.f);
    } else if (op == OP_LEADER || op == OP_COUNT || op == OP_STEP || op == OP_SIZE_FULL) {
        ok = B >= 1 && B <= dfm::CL_MAX_POSES && in(S_MASK, B * W32 * 4);
        if (op != OP_COUNT) {
            ok = ok && c->max_clusters >= 1 && in(S_ORDER, B * 4);
            if (op != OP_LEADER) ok = ok && in(S_POS, B * 4);
            if (ok) {      // order a permutation of 0..B-1, pos its inverse
                const int32_t *o = (const int32_t *)c->buf[S_ORDER].host;
                const int32_t *p = op != OP_LEADER ? (const int32_t *)c->buf[S_POS].host : nullptr;
                std::vector<char> seen((size_t)B, 0);
                for (long long i = 0; i < B && ok; ++i) {
                    ok = o[i] >= 0 && o[i] < B && !seen[(size_t)o[i]] && (!p || p[o[i]] == i);
                    if (ok) seen[(size_t)o[i]] = 1;
                }
            }
        }
        if (op == OP_LEADER) ok = ok && out(S_CLUSTER_OF, B * 4) && out(S_CENTER, maxc * 4) && out(S_SIZE, maxc * 4) && out(S_N_OUT, 4);
        if (op == OP_COUNT) ok = ok && out(S_COUNTS, B * 4) && out(S_U, W32 * 4) && out(S_CLUSTER_OF, B * 4) && out(S_STATE, 12);
        if (op == OP_SIZE_FULL)
            ok = ok && out(S_COUNTS, B * 4) && out(S_U, W32 * 4) && out(S_CLUSTER_OF, B * 4) && out(S_STATE, 12) && out(S_CENTER, maxc * 4) &&
                 out(S_SIZE, maxc * 4) && out(S_MLIST, B * 4);
        if (op == OP_STEP) {
            ok = ok && io(S_COUNTS, B * 4) && io(S_U, W32 * 4) && io(S_CLUSTER_OF, B * 4) && io(S_STATE, 12) && io(S_CENTER, maxc * 4) &&
                 io(S_SIZE, maxc * 4) && io(S_MLIST, B * 4);
            if (ok) {      // what the kernels index with: the cluster number, and the poses U names
                const int32_t *st = (const int32_t *)interior(S_STATE);
                const uint32_t *U = (const uint32_t *)interior(S_U);
                ok = (st[1] != 0 || (st[0] >= 0 && st[0] < maxc)) && st[2] >= 0 && st[2] <= B;
                if (ok && B % 32) ok = (U[W32 - 1] >> (B % 32)) == 0;
            }
        }
    } else if (op == OP_CONTACT_BITS || op == OP_CONTACT_COUNT || op == OP_CONTACT_SCORE || op == OP_CONSENSUS_FULL) {
        ok = n >= 1 && n <= MAX_CONSENSUS && R >= 1 && R <= MAX_CONSENSUS && L >= 1 && L <= MAX_CONSENSUS;
        const long long bits = n * W64 * R * 8;
        if (op == OP_CONTACT_BITS || op == OP_CONSENSUS_FULL) ok = ok && in(S_REC, R * 36) && in(S_LIG, n * L * 36) && out(S_BITS, bits) && c->cutoff > 0.f;
        else ok = ok && in(S_BITS, bits);
        if (ok && op != OP_CONTACT_BITS && op != OP_CONSENSUS_FULL && L % 64) {      // k_contact_score follows every set bit into count
            const uint64_t *b = (const uint64_t *)c->buf[S_BITS].host;
            for (long long p = 0; p < n && ok; ++p)
                for (long long i = 0; i < R && ok; ++i) ok = (b[(p * W64 + (W64 - 1)) * R + i] >> (L % 64)) == 0;
        }
        if (op == OP_CONTACT_COUNT || op == OP_CONSENSUS_FULL)
            ok = ok && in(S_MEMBER, n) && io(S_COUNT, R * L * 4) && io(S_REC_COUNT, R * 4) && io(S_LIG_COUNT, L * 4);
        if (op == OP_CONTACT_SCORE) ok = ok && in(S_COUNT, R * L * 4);
        if (op == OP_CONTACT_SCORE || op == OP_CONSENSUS_FULL) ok = ok && out(S_N_CONTACTS, n * 4) && out(S_SCORE_SUM, n * 8);
    } else {
        ok = false;
    }
    if (!ok) return (int)hipErrorInvalidValue;

    harness::Blocks<N_SLOTS> blk(c->buf);
    auto I = [&](int i) { return (int32_t *)blk.ptr(i); };
    const uint32_t *mask = (const uint32_t *)blk.ptr(S_MASK);
    const uint64_t *bits = (const uint64_t *)blk.ptr(S_BITS);

    hipStream_t s = nullptr;
    hipError_t e = blk.begin(&s);
    if (e == hipSuccess && (op == OP_POSE_RMSD || op == OP_POSE_MASK))
        e = dfm::launch_pose_dist((const float *)blk.ptr(S_X), c->B, c->L * 9, (const int32_t *)blk.ptr(S_RES), c->n_res, c->radius,
                                  op == OP_POSE_RMSD ? (float *)blk.ptr(S_RMSD) : nullptr, op == OP_POSE_MASK ? (uint32_t *)blk.ptr(S_MASK) : nullptr, s);
    if (e == hipSuccess && op == OP_LEADER)
        e = dfm::launch_cluster_leader(mask, c->B, I(S_ORDER), (int)maxc, I(S_CLUSTER_OF), I(S_CENTER), I(S_SIZE), I(S_N_OUT), s);
    if (e == hipSuccess && (op == OP_COUNT || op == OP_SIZE_FULL))
        e = dfm::launch_cluster_count(mask, c->B, I(S_COUNTS), (uint32_t *)blk.ptr(S_U), I(S_CLUSTER_OF), I(S_STATE), s);
    if (op == OP_STEP || op == OP_SIZE_FULL)
        for (long long k = 0; k < (op == OP_STEP ? 1 : maxc) && e == hipSuccess; ++k)
            e = dfm::launch_cluster_step(mask, c->B, I(S_COUNTS), I(S_POS), I(S_ORDER), (uint32_t *)blk.ptr(S_U), I(S_CLUSTER_OF), I(S_CENTER),
                                         I(S_SIZE), I(S_MLIST), I(S_STATE), s);
    if (e == hipSuccess && (op == OP_CONTACT_BITS || op == OP_CONSENSUS_FULL))
        e = dfm::launch_contact_bits((const float *)blk.ptr(S_REC), (const float *)blk.ptr(S_LIG), c->n, c->R, c->L, c->cutoff, (uint64_t *)blk.ptr(S_BITS), s);
    if (e == hipSuccess && (op == OP_CONTACT_COUNT || op == OP_CONSENSUS_FULL))
        e = dfm::launch_contact_count(bits, (const uint8_t *)blk.ptr(S_MEMBER), c->n, c->R, c->L, I(S_COUNT), I(S_REC_COUNT), I(S_LIG_COUNT), s);
    if (e == hipSuccess && (op == OP_CONTACT_SCORE || op == OP_CONSENSUS_FULL))
        e = dfm::launch_contact_score(bits, I(S_COUNT), c->n, c->R, c->L, I(S_N_CONTACTS), (int64_t *)blk.ptr(S_SCORE_SUM), s);
    return (int)blk.finish(e);
}

}  // extern "C"
