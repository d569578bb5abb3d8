// kernels_sterics.hip - all-atom clash and contact screen of P rigid ligand poses (include/dfmdock_amd.h: dfm_atoms_create /
// dfm_pose_sterics; the float64 numpy definition is dfmdock_amd/sterics.py).
//
// A pose is 24 bytes: (rot, tr) of the sampler.  Pose p of ligand atom a is (a - center) R(rot_p)^T + center + tr_p in fp64; a pair
// (receptor atom b, ligand atom a) is a contact when d = sqrt((dx*dx + dy*dy) + dz*dz), fp64 on the widened fp32 receptor atom and the
// fp64 ligand atom, is below the contact cutoff, a clash when below the clash cutoff.  Everything after that decision is an integer or a
// minimum, so no result depends on the order of the poses, on the blocks or on the chunks of a call.
//
// What dfm_atoms_create leaves on the device: the receptor atoms sorted by cell of a uniform grid whose edge is the contact cutoff
// (cell = (z ny + y) nx + x, so the cells x0 .. x1 of one (y, z) row are ONE contiguous range of atoms) with the cell starts; the ligand
// atoms sorted by the Morton code of their cell in the ligand's own frame, so that 64 consecutive atoms are a compact lump, with their
// index in the caller's order; per block of 64 ligand atoms a bounding sphere about the rotation centre's frame.
//
//   k_sterics_pose   one lane per pose: R(rot) in fp64 from the axis-angle, pdbio.axis_angle_to_matrix operation by operation (small-angle
//                    branch included), kept with tr as 12 doubles; zeroes the pose's counters, min_dist = +inf.
//   k_sterics        one wave per (pose, block of 64 ligand atoms).  In this order:
//                    1. a pose whose 12 doubles are not all finite is left at 0, 0, +inf (the definition: a NaN distance is nothing);
//                    2. the block's sphere, moved by the pose, against the receptor's bounding box grown by the cutoff: most blocks of
//                       most poses are nowhere near the receptor and the whole wave leaves here, having loaded 16 bytes;
//                    3. each lane transforms its atom in fp64 and keeps an fp32 copy; the block's exact bounding box (fp64 wave
//                       min / max) against the grown box once more, then its range of cells;
//                    4. for every (y, z) row of that range the row's atoms are staged in LDS, 64 at a time by one coalesced load, and
//                       read back as broadcasts (every lane reads the same address: no bank conflict, one ds_read_b128 per receptor
//                       atom for 64 pairs).  Letting each lane walk its own 27 cells instead would test about a sixth of the pairs, but
//                       with 64 different cell ranges per wave: every load a scattered gather, every loop as long as the wave's longest
//                       lane.  The staged form keeps the wave converged up to the fp64 branch, which few pairs take.
//                    5. per pair a conservative fp32 reject, then the fp64 distance decides against both cutoffs; counters are integers
//                       in registers, min_dist a wave minimum in fp64; one integer atomic per block and total, and an atomic minimum on
//                       the bits of the non-negative double (which order like the doubles).
//
// The fp32 reject: a pair is dropped without the fp64 arithmetic only when d2 > (contact * 1.0001f + slack)^2 with d2 taken in fp32 from
// the fp32 copy of the ligand atom; written as !(d2 > ...) for the pairs that go on, so a NaN goes on.  Why that is conservative: a pair
// below the cutoff has its ligand atom inside the receptor's box grown by the cutoff, so every coordinate involved is at most `maxabs` =
// the largest |coordinate| of that grown box.  The fp32 copy is off by at most 2^-24 maxabs per axis, the three differences and d2 add
// relative errors of a few 2^-24, so the fp32 distance is off by at most sqrt(3) 2^-24 maxabs + 4e-7 d < 1.04e-7 maxabs + 2e-6 (d <= 5).
// slack = max(1e-3, 2.5e-7 maxabs) A is above the first term at any scale (it stays 1e-3 A up to maxabs = 4000 A, which holds every
// PDB file), and the factor 1.0001 (5e-4 A at 5 A) is above the second.  The same slack grows the box tests of steps 2 and 3, which are taken in
// fp64; the cell of a coordinate is floor((x - origin) / edge) in fp64 here and on the host, a monotone function of x, so a receptor
// atom within the cutoff of the block's box can not lie in a cell below or above the block's range.
#include "dfm_internal.h"

namespace dfm {

namespace {

constexpr unsigned long long INF_BITS = 0x7FF0000000000000ull;

__device__ inline double wave_min(double v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}

__device__ inline double wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// cell coordinate of x along one axis, clamped to the grid: the host's binning formula
__device__ inline int cell_of(double x, double origin, double edge, int n)
{
    double c = floor((x - origin) / edge);
    c = c < 0.0 ? 0.0 : (c > (double)(n - 1) ? (double)(n - 1) : c);
    return (int)c;
}

}  // namespace

__global__ __launch_bounds__(64) void k_sterics_pose(const float *__restrict__ rot, const float *__restrict__ tr, int n, double *__restrict__ T,
                                                     int32_t *__restrict__ n_clash, int32_t *__restrict__ n_contact,
                                                     unsigned long long *__restrict__ min_bits)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    const double x = (double)rot[3 * p], y = (double)rot[3 * p + 1], z = (double)rot[3 * p + 2];
    const double ang = sqrt((x * x + y * y) + z * z);
    const double s = fabs(ang) < 1e-6 ? 0.5 - ang * ang / 48.0 : sin(0.5 * ang) / ang;
    const double r = cos(0.5 * ang), i = x * s, j = y * s, k = z * s;
    const double two_s = 2.0 / (((r * r + i * i) + j * j) + k * k);
    double *__restrict__ t = T + (int64_t)p * 12;
    t[0] = 1.0 - two_s * (j * j + k * k); t[1] = two_s * (i * j - k * r);       t[2] = two_s * (i * k + j * r);
    t[3] = two_s * (i * j + k * r);       t[4] = 1.0 - two_s * (i * i + k * k); t[5] = two_s * (j * k - i * r);
    t[6] = two_s * (i * k - j * r);       t[7] = two_s * (j * k + i * r);       t[8] = 1.0 - two_s * (i * i + j * j);
    t[9] = (double)tr[3 * p]; t[10] = (double)tr[3 * p + 1]; t[11] = (double)tr[3 * p + 2];
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
    const int lane = threadIdx.x, blk = blockIdx.x, p = blockIdx.y;
    double t[12], chk = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        t[k] = T[(int64_t)p * 12 + k];
        chk += t[k] * 0.0;
    }
    if (chk != chk) return;      // a NaN or infinite transform: 0, 0, +inf
    {
        const float4 bs = sphere[blk];
        const double qx = (double)bs.x, qy = (double)bs.y, qz = (double)bs.z, reach = (double)bs.w + sc.grow;
        const double cx = ((qx * t[0] + qy * t[1]) + qz * t[2]) + sc.center[0] + t[9];
        const double cy = ((qx * t[3] + qy * t[4]) + qz * t[5]) + sc.center[1] + t[10];
        const double cz = ((qx * t[6] + qy * t[7]) + qz * t[8]) + sc.center[2] + t[11];
        const double ex = cx < sc.lo[0] ? sc.lo[0] - cx : (cx > sc.hi[0] ? cx - sc.hi[0] : 0.0);
        const double ey = cy < sc.lo[1] ? sc.lo[1] - cy : (cy > sc.hi[1] ? cy - sc.hi[1] : 0.0);
        const double ez = cz < sc.lo[2] ? sc.lo[2] - cz : (cz > sc.hi[2] ? cz - sc.hi[2] : 0.0);
        if ((ex * ex + ey * ey) + ez * ez > reach * reach) {
            if (exits && lane == 0) atomicAdd(exits, 1ull);
            return;
        }
    }
    const int a = blk * 64 + lane;
    const bool valid = a < Al;
    const float4 l4 = lig[valid ? a : Al - 1];
    const double qx = (double)l4.x - sc.center[0], qy = (double)l4.y - sc.center[1], qz = (double)l4.z - sc.center[2];
    const double X = ((qx * t[0] + qy * t[1]) + qz * t[2]) + sc.center[0] + t[9];
    const double Y = ((qx * t[3] + qy * t[4]) + qz * t[5]) + sc.center[1] + t[10];
    const double Z = ((qx * t[6] + qy * t[7]) + qz * t[8]) + sc.center[2] + t[11];
    // (the lanes past Al repeat the last atom: they change no minimum or maximum)
    const double x0 = wave_min(X) - sc.grow, x1 = wave_max(X) + sc.grow;
    const double y0 = wave_min(Y) - sc.grow, y1 = wave_max(Y) + sc.grow;
    const double z0 = wave_min(Z) - sc.grow, z1 = wave_max(Z) + sc.grow;
    if (x0 > sc.hi[0] || x1 < sc.lo[0] || y0 > sc.hi[1] || y1 < sc.lo[1] || z0 > sc.hi[2] || z1 < sc.lo[2]) {
        if (exits && lane == 0) atomicAdd(exits + 1, 1ull);
        return;
    }
    // wave-uniform by construction; readfirstlane tells the compiler so (scalar loop control and scalar loads of the cell starts)
    const int cx0 = __builtin_amdgcn_readfirstlane(cell_of(x0, sc.lo[0], sc.edge, sc.nx));
    const int cx1 = __builtin_amdgcn_readfirstlane(cell_of(x1, sc.lo[0], sc.edge, sc.nx));
    const int cy0 = __builtin_amdgcn_readfirstlane(cell_of(y0, sc.lo[1], sc.edge, sc.ny));
    const int cy1 = __builtin_amdgcn_readfirstlane(cell_of(y1, sc.lo[1], sc.edge, sc.ny));
    const int cz0 = __builtin_amdgcn_readfirstlane(cell_of(z0, sc.lo[2], sc.edge, sc.nz));
    const int cz1 = __builtin_amdgcn_readfirstlane(cell_of(z1, sc.lo[2], sc.edge, sc.nz));
    const float xf = (float)X, yf = (float)Y, zf = (float)Z;
    int nc = 0, nt = 0;
    double dmin = __longlong_as_double((long long)INF_BITS);
    for (int cz = cz0; cz <= cz1; ++cz)
        for (int cy = cy0; cy <= cy1; ++cy) {
            const int row = (cz * sc.ny + cy) * sc.nx;
            const int b0 = cell_start[row + cx0], b1 = cell_start[row + cx1 + 1];
            for (int base = b0; base < b1; base += 64) {
                const int cnt = b1 - base < 64 ? b1 - base : 64;
                __syncthreads();      // the previous batch has been read
                if (lane < cnt) s_rec[lane] = rec[base + lane];
                __syncthreads();
                for (int j = 0; j < cnt; ++j) {
                    const float4 r = s_rec[j];
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
                }
            }
        }
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
