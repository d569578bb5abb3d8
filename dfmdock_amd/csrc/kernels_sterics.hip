// kernels_sterics.hip - all-atom clash and contact screen of P rigid ligand poses (include/dfmdock_amd.h: dfm_atoms_create /
// dfm_pose_sterics; the float64 numpy definition is dfmdock_amd/sterics.py).
//
// A pair (receptor atom b, ligand atom a of a pose) is a contact when d = sqrt((dx*dx + dy*dy) + dz*dz), fp64 on the widened fp32 receptor
// atom and the fp64 ligand atom, is below the contact cutoff, a clash when below the clash cutoff.  Everything after that decision is an
// integer or a minimum, so no result depends on the order of the poses, on the blocks or on the chunks of a call.
//
// What dfm_atoms_create leaves on the device: the receptor atoms sorted by cell of a uniform grid whose edge is the contact cutoff, with
// the cell starts; the ligand atoms sorted by the Morton code of their cell in the ligand's own frame, so that 64 consecutive atoms are
// a compact lump, with their index in the caller's order; per block of 64 ligand atoms a bounding sphere about the rotation centre's frame.
//
//   k_sterics_pose   one lane per pose: the pose as 12 doubles (dfm_posewalk.h: pose_transform); zeroes the pose's counters, min_dist = +inf.
//   k_sterics        one wave per (pose, block of 64 ligand atoms): the early exits and the staged receptor cell walk of dfm_posewalk.h,
//                    which also derives the fp32 reject.  Per pair that reject against the fp32 copy of the lane's atom, then the fp64
//                    distance decides against both cutoffs; counters are integers in registers, min_dist a wave minimum in fp64; one
//                    integer atomic per block and total, and an atomic minimum on the bits of the non-negative double (which order like
//                    the doubles).  A wave that leaves early leaves the pose at 0, 0, +inf.
#include "dfm_internal.h"
#include "dfm_posewalk.h"

namespace dfm {

namespace {

constexpr unsigned long long INF_BITS = 0x7FF0000000000000ull;

}  // namespace

__global__ __launch_bounds__(64) void k_sterics_pose(const float *__restrict__ rot, const float *__restrict__ tr, int n, double *__restrict__ T,
                                                     int32_t *__restrict__ n_clash, int32_t *__restrict__ n_contact,
                                                     unsigned long long *__restrict__ min_bits)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    pose_transform(rot, tr, p, T);
    n_clash[p] = 0;
    n_contact[p] = 0;
    min_bits[p] = INF_BITS;
}

// grid (blocks of 64 ligand atoms, poses of the chunk).  exits [2] (or nullptr): waves that left at the sphere test, at the box test
__global__ __launch_bounds__(64) void k_sterics(const float4 *__restrict__ rec, const int32_t *__restrict__ cell_start,
                                                const float4 *__restrict__ lig, const float4 *__restrict__ sphere,
                                                const int32_t *__restrict__ lig_index, const double *__restrict__ T, StericsConst sc, int Al,
                                                int32_t *__restrict__ n_clash, int32_t *__restrict__ n_contact,
                                                unsigned long long *__restrict__ min_bits, int32_t *__restrict__ lig_clash,
                                                int32_t *__restrict__ lig_contact, unsigned long long *__restrict__ exits)
{
    __shared__ float4 s_rec[64];
    const int lane = threadIdx.x, p = blockIdx.y, a = blockIdx.x * 64 + lane;
    WalkBlock w;
    if (!walk_front(sc.g, T, sphere, lig, Al, exits, w)) return;
    const bool valid = w.valid;
    const double X = w.X, Y = w.Y, Z = w.Z;
    const float xf = (float)X, yf = (float)Y, zf = (float)Z;
    int nc = 0, nt = 0;
    double dmin = __longlong_as_double((long long)INF_BITS);
    walk_rows(sc.g, w, cell_start, rec, s_rec, [&](int, const float4 r) {
        const float dx = r.x - xf, dy = r.y - yf, dz = r.z - zf;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (valid && !(d2 > sc.reject2)) {
            const double ex = X - (double)r.x, ey = Y - (double)r.y, ez = Z - (double)r.z;
            const double d = sqrt((ex * ex + ey * ey) + ez * ez);
            if (d < sc.contact) {
                ++nt;
                nc += d < sc.clash ? 1 : 0;
                dmin = d < dmin ? d : dmin;
            }
        }
    });
    if (lig_clash && valid) lig_clash[(int64_t)p * Al + lig_index[a]] = nc;
    if (lig_contact && valid) lig_contact[(int64_t)p * Al + lig_index[a]] = nt;
    for (int o = 32; o > 0; o >>= 1) {
        nc += __shfl_xor(nc, o);
        nt += __shfl_xor(nt, o);
    }
    dmin = wave_min(dmin);
    if (lane == 0 && nt != 0) {
        atomicAdd(n_contact + p, nt);
        if (nc != 0) atomicAdd(n_clash + p, nc);
        atomicMin(min_bits + p, (unsigned long long)__double_as_longlong(dmin));
    }
}

hipError_t launch_sterics_pose(const float *rot, const float *tr, int n, double *T, int32_t *n_clash, int32_t *n_contact, uint64_t *min_bits,
                               hipStream_t s)
{
    hipLaunchKernelGGL(k_sterics_pose, dim3((unsigned)((n + 63) / 64)), dim3(64), token_lds(), s, rot, tr, n, T, n_clash, n_contact,
                       reinterpret_cast<unsigned long long *>(min_bits));
    return hipGetLastError();
}

hipError_t launch_sterics(const StericsAtoms &at, const double *T, int n, int32_t *n_clash, int32_t *n_contact, uint64_t *min_bits,
                          int32_t *lig_clash, int32_t *lig_contact, uint64_t *exits, hipStream_t s)
{
    if (n < 1 || n > 65535) return hipErrorInvalidValue;      // poses are gridDim.y
    hipLaunchKernelGGL(k_sterics, dim3((unsigned)((at.Al + 63) / 64), (unsigned)n), dim3(64), token_lds(), s,
                       reinterpret_cast<const float4 *>(at.rec), at.cell_start, reinterpret_cast<const float4 *>(at.lig),
                       reinterpret_cast<const float4 *>(at.sphere), at.lig_index, T, at.sc, at.Al, n_clash, n_contact,
                       reinterpret_cast<unsigned long long *>(min_bits), lig_clash, lig_contact,
                       reinterpret_cast<unsigned long long *>(exits));
    return hipGetLastError();
}

}  // namespace dfm
