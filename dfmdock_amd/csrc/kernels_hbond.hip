// kernels_hbond.hip - interface hydrogen bonds and salt bridges of P rigid ligand poses over the POLAR atoms of the two chains
// (include/dfmdock_amd.h: dfm_hbond_create / dfm_pose_hbonds; the float64 numpy definition is dfmdock_amd/hbonds.py).
//
// Heavy atoms only: a pair is a hydrogen bond when its roles are complementary, its squared distance is below hb_cutoff^2 and the angles
// at both atoms, taken to their antecedents, are at least min_angle - written without a square root or a division as
// du <= 0 and du*du >= c2 (uu r2), in fp64 on the widened fp32 receptor atom and the fp64 posed ligand atom, in the definition's order
// of operations (the file is built with floating-point contraction off).  A cation / anion pair below salt_cutoff^2 is a salt-bridge
// atom pair; the salt BRIDGES of a pose are the distinct residue pairs those make, found by many lanes, waves and blocks, so a pose has
// a bitmap [Lc][Wc] of 32-bit words over the charged residues of the two chains (Wc = ceil(Rc / 32)), as in kernels_rescon.hip.
// Everything after the comparisons is an integer and OR commutes: no result depends on the order of the poses, the blocks or the chunks.
//
//   k_hbond_pose      one lane per pose: the pose as 12 doubles (dfm_posewalk.h: pose_transform), the pose's five totals zeroed.
//   k_hbond           one wave per (pose, block of 64 ligand polar atoms): the early exits of walk_front, then the lane poses its atom's
//                     antecedent with the same t[12], and the two-array cell walk stages each receptor atom with its antecedent.  Per
//                     pair the shared fp32 reject at the larger cutoff, then the roles (integers: most pairs of polar atoms are not
//                     complementary and stop here), then the fp64 tests.  A lane counts in registers; the wave sums and lane 0 adds the
//                     four sums to the pose's totals with one integer atomicAdd each.  The receptor's per-atom counts are integer
//                     atomicAdds (few pairs pass); the ligand's are the lane's own registers, stored once.  A salt-bridge pair sets its
//                     residue pair's bit as k_rescon does.
//   k_hbond_finish    one wave per pose: the popcount of its bitmap = n_salt.
#include "dfm_internal.h"
#include "dfm_posewalk.h"

namespace dfm {

namespace {

__device__ __forceinline__ int wave_sum_i(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace

// tot [n][5] = bonds with 0, 1, 2 side-chain atoms, salt-bridge atom pairs, salt bridges
__global__ __launch_bounds__(64) void k_hbond_pose(const float *__restrict__ rot, const float *__restrict__ tr, int n, double *__restrict__ T,
                                                   int32_t *__restrict__ tot)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    pose_transform(rot, tr, p, T);
#pragma unroll
    for (int k = 0; k < 5; ++k) tot[(int64_t)p * 5 + k] = 0;
}

// grid (blocks of 64 ligand polar atoms, poses of the chunk).  bits [poses][Lc][Wc], zeroed; the per-atom arrays [poses][Nr] / [poses][Nl]
// (the caller's atom order) or nullptr, zeroed
__global__ __launch_bounds__(64) void k_hbond(const float4 *__restrict__ rec, const float4 *__restrict__ rec_ante,
                                              const int32_t *__restrict__ cell_start, const int32_t *__restrict__ rec_index,
                                              const float4 *__restrict__ lig, const float4 *__restrict__ lig_ante,
                                              const int32_t *__restrict__ lig_index, const float4 *__restrict__ sphere,
                                              const double *__restrict__ T, HbondConst sc, int Nr, int Nl, int Lc, int Wc, int32_t *tot,
                                              uint32_t *bits, int32_t *rec_hb, int32_t *rec_sb, int32_t *__restrict__ lig_hb,
                                              int32_t *__restrict__ lig_sb)
{
    __shared__ float4 s_rec[64], s_ante[64];
    const int p = blockIdx.y;
    WalkBlock w;
    if (!walk_front(sc.g, T, sphere, lig, Nl, nullptr, w)) return;
    const bool valid = w.valid;
    const int a = valid ? (int)(blockIdx.x * 64 + threadIdx.x) : Nl - 1;
    const double X = w.X, Y = w.Y, Z = w.Z;
    const float xf = (float)X, yf = (float)Y, zf = (float)Z;
    // the antecedent rides with the ligand: the same transform
    double ux, uy, uz, uu;
    {
        const float4 la = lig_ante[a];
        const double *t = w.t;
        const double qx = (double)la.x - sc.g.center[0], qy = (double)la.y - sc.g.center[1], qz = (double)la.z - sc.g.center[2];
        ux = (((qx * t[0] + qy * t[1]) + qz * t[2]) + sc.g.center[0] + t[9]) - X;
        uy = (((qx * t[3] + qy * t[4]) + qz * t[5]) + sc.g.center[1] + t[10]) - Y;
        uz = (((qx * t[6] + qy * t[7]) + qz * t[8]) + sc.g.center[2] + t[11]) - Z;
        uu = (ux * ux + uy * uy) + uz * uz;
    }
    const uint32_t lb = (uint32_t)__float_as_int(w.l4.w);
    const bool l_don = lb & HB_DONOR, l_acc = lb & HB_ACCEPTOR, l_cat = lb & HB_CATION, l_an = lb & HB_ANION;
    const int l_side = (int)((lb >> 4) & 1u);
    // an atom without a charge carries residue 0 and never reads its row
    uint32_t *row = bits + ((int64_t)p * Lc + (int)(lb >> HB_RES_SHIFT)) * Wc;
    int32_t *r_hb = rec_hb ? rec_hb + (int64_t)p * Nr : nullptr, *r_sb = rec_sb ? rec_sb + (int64_t)p * Nr : nullptr;
    int k0 = 0, k1 = 0, k2 = 0, n_sa = 0, last = -1;
    walk_rows(sc.g, w, cell_start, rec, rec_ante, s_rec, s_ante, [&](int q, const float4 r, const float4 ra) {
        const float fx = r.x - xf, fy = r.y - yf, fz = r.z - zf;
        const float d2 = (fx * fx + fy * fy) + fz * fz;
        if (valid && !(d2 > sc.reject2)) {
            const uint32_t rb = (uint32_t)__float_as_int(r.w);
            const bool compl_ = (l_don && (rb & HB_ACCEPTOR)) || (l_acc && (rb & HB_DONOR));
            const bool ionic = (l_cat && (rb & HB_ANION)) || (l_an && (rb & HB_CATION));
            if (compl_ || ionic) {
                const double px = (double)r.x, py = (double)r.y, pz = (double)r.z;
                const double dx = px - X, dy = py - Y, dz = pz - Z;
                const double r2 = (dx * dx + dy * dy) + dz * dz;
                if (ionic && r2 < sc.salt2) {
                    ++n_sa;
                    if (r_sb) atomicAdd(r_sb + rec_index[q], 1);
                    const int i = (int)(rb >> HB_RES_SHIFT);
                    if (i != last) {
                        last = i;
                        uint32_t *word = row + (i >> 5);
                        const uint32_t bit = 1u << (i & 31);
                        if (!(__atomic_load_n(word, __ATOMIC_RELAXED) & bit)) atomicOr(word, bit);
                    }
                }
                if (compl_ && r2 < sc.hb2) {
                    const double du = (ux * dx + uy * dy) + uz * dz;
                    if (du <= 0.0 && du * du >= sc.c2 * (uu * r2)) {
                        const double wx = (double)ra.x - px, wy = (double)ra.y - py, wz = (double)ra.z - pz;
                        const double ww = (wx * wx + wy * wy) + wz * wz;
                        const double dw = -((wx * dx + wy * dy) + wz * dz);
                        if (dw <= 0.0 && dw * dw >= sc.c2 * (ww * r2)) {
                            const int kind = l_side + (int)((rb >> 4) & 1u);
                            k0 += kind == 0 ? 1 : 0;
                            k1 += kind == 1 ? 1 : 0;
                            k2 += kind == 2 ? 1 : 0;
                            if (r_hb) atomicAdd(r_hb + rec_index[q], 1);
                        }
                    }
                }
            }
        }
    });
    if (valid && (lig_hb || lig_sb)) {      // this wave alone owns the atom
        const int64_t at = (int64_t)p * Nl + lig_index[a];
        if (lig_hb) lig_hb[at] = (k0 + k1) + k2;
        if (lig_sb) lig_sb[at] = n_sa;
    }
    k0 = wave_sum_i(k0);
    k1 = wave_sum_i(k1);
    k2 = wave_sum_i(k2);
    n_sa = wave_sum_i(n_sa);
    if (threadIdx.x == 0) {
        int32_t *o = tot + (int64_t)p * 5;
        if (k0) atomicAdd(o, k0);
        if (k1) atomicAdd(o + 1, k1);
        if (k2) atomicAdd(o + 2, k2);
        if (n_sa) atomicAdd(o + 3, n_sa);
    }
}

// grid (poses of the chunk).  words = Lc Wc words of bitmap per pose (0: no charged residue in one of the chains)
__global__ __launch_bounds__(64) void k_hbond_finish(const uint32_t *__restrict__ bits, int words, int32_t *__restrict__ tot)
{
    const int lane = threadIdx.x, p = blockIdx.x;
    const uint32_t *b = bits + (int64_t)p * words;
    int c = 0;
    for (int i = lane; i < words; i += 64) c += __popc(b[i]);
    c = wave_sum_i(c);
    if (lane == 0) tot[(int64_t)p * 5 + 4] = c;
}

hipError_t launch_hbond_pose(const float *rot, const float *tr, int n, double *T, int32_t *tot, hipStream_t s)
{
    hipLaunchKernelGGL(k_hbond_pose, dim3((unsigned)((n + 63) / 64)), dim3(64), token_lds(), s, rot, tr, n, T, tot);
    return hipGetLastError();
}

hipError_t launch_hbond(const HbondAtoms &at, const double *T, int n, int32_t *tot, uint32_t *bits, int32_t *rec_hb, int32_t *rec_sb,
                        int32_t *lig_hb, int32_t *lig_sb, hipStream_t s)
{
    if (n < 1 || n > 65535) return hipErrorInvalidValue;      // poses are gridDim.y
    hipLaunchKernelGGL(k_hbond, dim3((unsigned)((at.Nl + 63) / 64), (unsigned)n), dim3(64), token_lds(), s,
                       reinterpret_cast<const float4 *>(at.rec), reinterpret_cast<const float4 *>(at.rec_ante), at.cell_start, at.rec_index,
                       reinterpret_cast<const float4 *>(at.lig), reinterpret_cast<const float4 *>(at.lig_ante), at.lig_index,
                       reinterpret_cast<const float4 *>(at.sphere), T, at.sc, at.Nr, at.Nl, at.Lc, at.Wc, tot, bits, rec_hb, rec_sb, lig_hb,
                       lig_sb);
    return hipGetLastError();
}

hipError_t launch_hbond_finish(const HbondAtoms &at, const uint32_t *bits, int n, int32_t *tot, hipStream_t s)
{
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hbond_finish, dim3((unsigned)n), dim3(64), token_lds(), s, bits, at.Lc * at.Wc, tot);
    return hipGetLastError();
}

}  // namespace dfm
