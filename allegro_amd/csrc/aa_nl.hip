// On-device neighbor list: cell list -> center-sorted CSR edge list (center, nbr, rowptr, periodic shifts) -- the
// graph contract of the hot path (aa_graph), built without leaving the GPU.  In the reference
// stack the list comes from the host (nequip's neighbor-list transform, EXT) or from LAMMPS (pair_allegro); the
// conventions are those of `with_edge_vectors_` (called at allegro/nn/tensorembed.py:86):
//     r_e = pos[nbr] - pos[center] + cell_shift_e @ cell,   |r_e| < r_cut,   self-pairs only through a non-zero shift.
// Geometry is evaluated in double for either position dtype so that borderline pairs are classified the same way as
// by a float64 host list.  Deterministic: cells are filled with integer atomics and then sorted, neighbors of an
// atom are emitted in (cell offset, atom index) order.
#include "aa_common.h"

#include <algorithm>
#include <cmath>

using namespace aa;
namespace {

struct NlDev {
  int64_t N;
  const void* pos;
  double cell[9], inv[9];
  int nc[3], k[3], pbc[3];
  double rc2;
  int ncells;
  // workspace
  int* cell_count;  // [ncells+1]
  int* cell_start;  // [ncells+1]
  int* atom_cell;   // [N]
  int* atom_slot;   // [N]
  int* cell_atoms;  // [N]
  int* wrap;        // [N][3]
  double* wpos;     // [N][3] positions wrapped into the cell along periodic directions
  int* counts;      // [N+1]
  int* scan_tmp;    // [max(cells, atoms) / 4096 + 2]
};

// per-type-pair cutoffs (aa_nl_types) as the kernels see them; the untyped instantiations never touch it
constexpr int kMaxTypes = 64;  // the squared table sits in LDS as doubles: 64 * 64 * 8 = 32 KB
struct NlTypesDev {
  const void* atom_types;  // [N] the caller's int32 / int64 array
  int* wtype;              // [N] workspace: the types as int32, clamped into [0, T)
  const double* rc2;       // [T,T] workspace: min(r_cut, table)^2
  int* bad_type;           // workspace: set to 1 by any atom whose type was clamped
  int T;
};
// the caller's type of atom i as an index into the table: never outside it, whatever the array holds
template <typename TT>
__device__ __forceinline__ int clamped_type(const void* atom_types, int64_t i, int T, int* bad_type) {
  const TT t = static_cast<const TT*>(atom_types)[i];
  if (t < 0 || t >= TT(T)) {
    *bad_type = 1;
    return t < 0 ? 0 : T - 1;
  }
  return int(t);
}

// TYPES: 0 = untyped list, 1 / 2 = the atom types (int32 / int64) are binned into the workspace next to wpos as int32, so that
// the caller's array is read once and the pair loop reads a compact one
template <typename T, int TYPES = 0>
__global__ __launch_bounds__(256) void nl_bin_kernel(NlDev d, NlTypesDev ty) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= d.N) return;
  if constexpr (TYPES == 1) ty.wtype[i] = clamped_type<int32_t>(ty.atom_types, i, ty.T, ty.bad_type);
  if constexpr (TYPES == 2) ty.wtype[i] = clamped_type<int64_t>(ty.atom_types, i, ty.T, ty.bad_type);
  const T* p = static_cast<const T*>(d.pos) + 3 * i;
  const double x = double(p[0]), y = double(p[1]), z = double(p[2]);
  double s[3];
  int w[3], c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    s[a] = x * d.inv[0 * 3 + a] + y * d.inv[1 * 3 + a] + z * d.inv[2 * 3 + a];
    w[a] = 0;
    if (d.pbc[a]) {
      const double fl = floor(s[a]);
      w[a] = -int(fl);
      s[a] -= fl;
      if (s[a] >= 1.0) {  // rounding: -1e-17 - floor(.) == 1.0
        s[a] -= 1.0;
        w[a] -= 1;
      }
    }
    int ca = int(floor(s[a] * d.nc[a]));
    c[a] = ca < 0 ? 0 : (ca >= d.nc[a] ? d.nc[a] - 1 : ca);  // atoms outside a non-periodic box go to the border cells
  }
  d.wpos[3 * i + 0] = x + w[0] * d.cell[0] + w[1] * d.cell[3] + w[2] * d.cell[6];
  d.wpos[3 * i + 1] = y + w[0] * d.cell[1] + w[1] * d.cell[4] + w[2] * d.cell[7];
  d.wpos[3 * i + 2] = z + w[0] * d.cell[2] + w[1] * d.cell[5] + w[2] * d.cell[8];
  d.wrap[3 * i + 0] = w[0];
  d.wrap[3 * i + 1] = w[1];
  d.wrap[3 * i + 2] = w[2];
  const int cid = (c[0] * d.nc[1] + c[1]) * d.nc[2] + c[2];
  d.atom_cell[i] = cid;
  d.atom_slot[i] = atomicAdd(&d.cell_count[cid], 1);
}

// Exclusive prefix sums out[0..n] of in[0..n) (out[n] = total) in three launches: per-block totals (4096 items per
// workgroup), one workgroup scans the totals, every workgroup scans its own items from its offset.
constexpr int kScanItems = 16, kScanBlock = 256 * kScanItems;

__global__ __launch_bounds__(256) void nl_scan_totals_kernel(const int* in, int* block_tot, int64_t n) {
  int* sSum = reinterpret_cast<int*>(aa_smem);  // [256]
  const int tid = threadIdx.x;
  const int64_t lo = int64_t(blockIdx.x) * kScanBlock + int64_t(tid) * kScanItems;
  int acc = 0;
  for (int q = 0; q < kScanItems; ++q)
    if (lo + q < n) acc += in[lo + q];
  sSum[tid] = acc;
  __syncthreads();
  for (int st = 128; st >= 1; st >>= 1) {
    if (tid < st) sSum[tid] += sSum[tid + st];
    __syncthreads();
  }
  if (tid == 0) block_tot[blockIdx.x] = sSum[0];
}

// in place: block_tot[b] -> sum of block_tot[0..b); out_total = grand total.  One workgroup, chunk per thread.
__global__ __launch_bounds__(256) void nl_scan_offsets_kernel(int* block_tot, int nblocks, int* out_total) {
  int* sSum = reinterpret_cast<int*>(aa_smem);
  const int tid = threadIdx.x;
  const int chunk = (nblocks + 255) / 256;
  const int lo = std::min(nblocks, chunk * tid), hi = std::min(nblocks, lo + chunk);
  int acc = 0;
  for (int q = lo; q < hi; ++q) acc += block_tot[q];
  sSum[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < 256; ++t) {
      const int v = sSum[t];
      sSum[t] = run;
      run += v;
    }
    *out_total = run;
  }
  __syncthreads();
  int run = sSum[tid];
  for (int q = lo; q < hi; ++q) {
    const int v = block_tot[q];
    block_tot[q] = run;
    run += v;
  }
}

__global__ __launch_bounds__(256) void nl_scan_apply_kernel(const int* in, const int* block_off, int* out, int64_t n) {
  int* sSum = reinterpret_cast<int*>(aa_smem);  // [256]
  const int tid = threadIdx.x;
  const int64_t lo = int64_t(blockIdx.x) * kScanBlock + int64_t(tid) * kScanItems;
  int v[kScanItems];
  int acc = 0;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    v[q] = lo + q < n ? in[lo + q] : 0;
    acc += v[q];
  }
  sSum[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    int run = block_off[blockIdx.x];
    for (int t = 0; t < 256; ++t) {
      const int x = sSum[t];
      sSum[t] = run;
      run += x;
    }
  }
  __syncthreads();
  int run = sSum[tid];
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    if (lo + q < n) out[lo + q] = run;
    run += v[q];
  }
}

// out[n] receives the total; `block_tot` is scratch of (n / 4096 + 1) ints
void launch_scan(const int* in, int* out, int64_t n, int* block_tot, hipStream_t s) {
  const int nb = int((n + kScanBlock - 1) / kScanBlock);
  if (nb > 0) hipLaunchKernelGGL(nl_scan_totals_kernel, dim3(nb), dim3(256), sizeof(int) * 256, s, in, block_tot, n);
  hipLaunchKernelGGL(nl_scan_offsets_kernel, dim3(1), dim3(256), sizeof(int) * 256, s, block_tot, nb, out + n);
  if (nb > 0) hipLaunchKernelGGL(nl_scan_apply_kernel, dim3(nb), dim3(256), sizeof(int) * 256, s, in, block_tot, out, n);
}

__global__ __launch_bounds__(256) void nl_cell_fill_kernel(NlDev d) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= d.N) return;
  d.cell_atoms[d.cell_start[d.atom_cell[i]] + d.atom_slot[i]] = int(i);
}

// the slots came from atomics: sort every cell's (short) atom list so that the edge order is reproducible
__global__ __launch_bounds__(256) void nl_cell_sort_kernel(NlDev d) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d.ncells) return;
  const int lo = d.cell_start[c], hi = d.cell_start[c + 1];
  for (int q = lo + 1; q < hi; ++q) {
    const int v = d.cell_atoms[q];
    int r = q - 1;
    while (r >= lo && d.cell_atoms[r] > v) {
      d.cell_atoms[r + 1] = d.cell_atoms[r];
      --r;
    }
    d.cell_atoms[r + 1] = v;
  }
}

// TYPED: the cutoff of a pair is sRc2[type_i][type_j] = min(r_cut, table)^2, doubles in LDS (the table is read once per candidate
// pair; 32 KB at the 64-type cap), instead of d.rc2.  The count (FILL = false) and the fill pass are the same code, so they apply
// the identical predicate -- same double arithmetic, same operand order -- and rowptr always matches what fill writes.  The
// untyped instantiation compiles to what it was before the flag existed.
template <typename T, bool FILL, bool TYPED = false>
__global__ __launch_bounds__(256) void nl_pairs_kernel(NlDev d, const int32_t* rowptr, int32_t* center, int32_t* nbr,
                                                       int32_t* cell_shift, void* shift_vec, NlTypesDev ty) {
  [[maybe_unused]] const double* sRow = nullptr;  // row type_i of the squared table
  if constexpr (TYPED) {
    double* sRc2 = reinterpret_cast<double*>(aa_smem);  // [T][T]
    for (int q = threadIdx.x; q < ty.T * ty.T; q += 256) sRc2[q] = ty.rc2[q];
    __syncthreads();
  }
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= d.N) return;
  if constexpr (TYPED) sRow = reinterpret_cast<const double*>(aa_smem) + ty.wtype[i] * ty.T;
  const double xi = d.wpos[3 * i], yi = d.wpos[3 * i + 1], zi = d.wpos[3 * i + 2];
  const int cid = d.atom_cell[i];
  const int c2 = cid % d.nc[2], c1 = (cid / d.nc[2]) % d.nc[1], c0 = cid / (d.nc[2] * d.nc[1]);
  const int wi0 = d.wrap[3 * i], wi1 = d.wrap[3 * i + 1], wi2 = d.wrap[3 * i + 2];
  int cnt = 0;
  int64_t e = FILL ? rowptr[i] : 0;
  for (int o0 = -d.k[0]; o0 <= d.k[0]; ++o0) {
    int a0 = c0 + o0, n0 = 0;
    if (d.pbc[0]) {
      n0 = a0 >= 0 ? a0 / d.nc[0] : -((-a0 + d.nc[0] - 1) / d.nc[0]);
      a0 -= n0 * d.nc[0];
    } else if (a0 < 0 || a0 >= d.nc[0]) {
      continue;
    }
    for (int o1 = -d.k[1]; o1 <= d.k[1]; ++o1) {
      int a1 = c1 + o1, n1 = 0;
      if (d.pbc[1]) {
        n1 = a1 >= 0 ? a1 / d.nc[1] : -((-a1 + d.nc[1] - 1) / d.nc[1]);
        a1 -= n1 * d.nc[1];
      } else if (a1 < 0 || a1 >= d.nc[1]) {
        continue;
      }
      for (int o2 = -d.k[2]; o2 <= d.k[2]; ++o2) {
        int a2 = c2 + o2, n2 = 0;
        if (d.pbc[2]) {
          n2 = a2 >= 0 ? a2 / d.nc[2] : -((-a2 + d.nc[2] - 1) / d.nc[2]);
          a2 -= n2 * d.nc[2];
        } else if (a2 < 0 || a2 >= d.nc[2]) {
          continue;
        }
        const double sx = n0 * d.cell[0] + n1 * d.cell[3] + n2 * d.cell[6];
        const double sy = n0 * d.cell[1] + n1 * d.cell[4] + n2 * d.cell[7];
        const double sz = n0 * d.cell[2] + n1 * d.cell[5] + n2 * d.cell[8];
        const int cj = (a0 * d.nc[1] + a1) * d.nc[2] + a2;
        const bool home = n0 == 0 && n1 == 0 && n2 == 0;
        for (int q = d.cell_start[cj]; q < d.cell_start[cj + 1]; ++q) {
          const int j = d.cell_atoms[q];
          if (home && j == i) continue;
          const double dx = d.wpos[3 * int64_t(j)] + sx - xi, dy = d.wpos[3 * int64_t(j) + 1] + sy - yi,
                       dz = d.wpos[3 * int64_t(j) + 2] + sz - zi;
          bool listed;
          if constexpr (TYPED)
            listed = dx * dx + dy * dy + dz * dz < sRow[ty.wtype[j]];
          else
            listed = dx * dx + dy * dy + dz * dz < d.rc2;
          if (listed) {
            if constexpr (FILL) {
              center[e] = int32_t(i);
              nbr[e] = j;
              // undo the wrapping: r_e = pos[j] - pos[i] + S @ cell with S = n + w_j - w_i
              const int S0 = n0 + d.wrap[3 * int64_t(j)] - wi0, S1 = n1 + d.wrap[3 * int64_t(j) + 1] - wi1,
                        S2 = n2 + d.wrap[3 * int64_t(j) + 2] - wi2;
              if (cell_shift) {
                cell_shift[3 * e] = S0;
                cell_shift[3 * e + 1] = S1;
                cell_shift[3 * e + 2] = S2;
              }
              if (shift_vec) {
                T* sv = static_cast<T*>(shift_vec) + 3 * e;
                sv[0] = T(S0 * d.cell[0] + S1 * d.cell[3] + S2 * d.cell[6]);
                sv[1] = T(S0 * d.cell[1] + S1 * d.cell[4] + S2 * d.cell[7]);
                sv[2] = T(S0 * d.cell[2] + S1 * d.cell[5] + S2 * d.cell[8]);
              }
              ++e;
            } else {
              ++cnt;
            }
          }
        }
      }
    }
  }
  if constexpr (!FILL) d.counts[i] = cnt;
}

size_t align_up(size_t x) { return (x + 255) / 256 * 256; }

int64_t max_cells(int64_t N) { return std::max<int64_t>(64, 4 * N); }

// `r_list`: the radius the cell grid is sized by and d.rc2 is set from -- r_cut, or min(r_cut, largest table entry) of a typed list
int plan_nl(const aa_nl_input* in, void* ws, size_t ws_bytes, size_t need_bytes, double r_list, NlDev& d) {
  AA_REQUIRE(in && ws, "aa_nl: null argument");
  AA_REQUIRE(in->num_atoms >= 0 && in->num_atoms < (int64_t(1) << 31), "aa_nl: atom count out of range");
  AA_REQUIRE(in->dtype == AA_F32 || in->dtype == AA_F64, "aa_nl: bad dtype");
  AA_REQUIRE(in->r_cut > 0.0, "aa_nl: r_cut must be positive");
  AA_REQUIRE(in->pos || in->num_atoms == 0, "aa_nl: null positions");
  if (ws_bytes < need_bytes) return fail(AA_ERR_WORKSPACE, "aa_nl: workspace too small");
  d.N = in->num_atoms;
  d.pos = in->pos;
  const double* c = in->cell;
  for (int q = 0; q < 9; ++q) d.cell[q] = c[q];
  const double det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
  AA_REQUIRE(std::fabs(det) > 1e-12, "aa_nl: singular cell");
  // inverse (pos = s @ cell  =>  s = pos @ inv)
  d.inv[0] = (c[4] * c[8] - c[5] * c[7]) / det;
  d.inv[1] = (c[2] * c[7] - c[1] * c[8]) / det;
  d.inv[2] = (c[1] * c[5] - c[2] * c[4]) / det;
  d.inv[3] = (c[5] * c[6] - c[3] * c[8]) / det;
  d.inv[4] = (c[0] * c[8] - c[2] * c[6]) / det;
  d.inv[5] = (c[2] * c[3] - c[0] * c[5]) / det;
  d.inv[6] = (c[3] * c[7] - c[4] * c[6]) / det;
  d.inv[7] = (c[1] * c[6] - c[0] * c[7]) / det;
  d.inv[8] = (c[0] * c[4] - c[1] * c[3]) / det;
  // perpendicular height of the cell along lattice direction a = 1 / |column a of inv|
  double h[3];
  for (int a = 0; a < 3; ++a) {
    const double n2 = d.inv[a] * d.inv[a] + d.inv[3 + a] * d.inv[3 + a] + d.inv[6 + a] * d.inv[6 + a];
    h[a] = 1.0 / std::sqrt(n2);
    d.pbc[a] = in->pbc[a] ? 1 : 0;
    d.nc[a] = std::max(1, int(std::min(1024.0, std::floor(h[a] / r_list))));
  }
  while (int64_t(d.nc[0]) * d.nc[1] * d.nc[2] > max_cells(d.N)) {  // never more cells than ~4 per atom
    int a = 0;
    if (d.nc[1] > d.nc[a]) a = 1;
    if (d.nc[2] > d.nc[a]) a = 2;
    d.nc[a] = (d.nc[a] + 1) / 2;
  }
  for (int a = 0; a < 3; ++a) {
    const double width = h[a] / d.nc[a];
    d.k[a] = d.pbc[a] ? int(std::ceil(r_list / width - 1e-12)) : (d.nc[a] > 1 ? 1 : 0);
    AA_REQUIRE(d.k[a] <= 64, "aa_nl: cell much smaller than r_cut (more than 64 images along one direction)");
  }
  d.rc2 = r_list * r_list;
  d.ncells = d.nc[0] * d.nc[1] * d.nc[2];
  char* base = static_cast<char*>(ws);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* r = base + o;
    o += align_up(bytes);
    return r;
  };
  const size_t N = size_t(d.N), NC = size_t(max_cells(d.N));
  d.cell_count = reinterpret_cast<int*>(take(sizeof(int) * (NC + 1)));
  d.cell_start = reinterpret_cast<int*>(take(sizeof(int) * (NC + 1)));
  d.atom_cell = reinterpret_cast<int*>(take(sizeof(int) * N));
  d.atom_slot = reinterpret_cast<int*>(take(sizeof(int) * N));
  d.cell_atoms = reinterpret_cast<int*>(take(sizeof(int) * N));
  d.wrap = reinterpret_cast<int*>(take(sizeof(int) * 3 * N));
  d.wpos = reinterpret_cast<double*>(take(sizeof(double) * 3 * N));
  d.counts = reinterpret_cast<int*>(take(sizeof(int) * (N + 1)));
  d.scan_tmp = reinterpret_cast<int*>(take(sizeof(int) * (std::max(N, NC) / kScanBlock + 2)));
  return AA_OK;
}

// ---- transposed CSR of a center-sorted edge list (edges grouped by NEIGHBOUR atom, ascending edge id inside a group = the stable
// ---- argsort of nbr) and the three graph hints, without leaving the device: counting sort by atomics + a per-atom sort of the
// ---- (short) groups, which makes the result independent of the order the atomics were served in
// (a neighbour id outside [0, N) -- a malformed list -- is skipped by both passes alike: its edge appears in no group, nothing is
//  written out of bounds; the step itself reads pos[nbr] and is the caller's to keep valid)
__global__ __launch_bounds__(256) void gt_count_kernel(const int32_t* nbr, int64_t E, int64_t N, int* cnt) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= E) return;
  const int j = nbr[e];
  if (j >= 0 && j < N) atomicAdd(&cnt[j], 1);
}
__global__ __launch_bounds__(256) void gt_place_kernel(const int32_t* nbr, int64_t E, int64_t N, const int32_t* t_rowptr, int* cursor,
                                                       int32_t* t_perm) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= E) return;
  const int j = nbr[e];
  if (j >= 0 && j < N) t_perm[t_rowptr[j] + atomicAdd(&cursor[j], 1)] = int32_t(e);
}
// one wave per atom: every entry's final position is its RANK inside the group (edge ids are distinct), counted with wave shuffles
// from registers -- no data-dependent loop over memory, whatever order the atomics left the group in (groups of more than 256
// entries: one lane sorts in place)
// (the body is a device function so that the list ingest, aa_graph_build_fill, ranks its center segments with the same code)
__device__ __forceinline__ void gt_sort_group(int lane, int64_t a, const int32_t* t_rowptr, int32_t* t_perm) {
  const int lo = __builtin_amdgcn_readfirstlane(t_rowptr[a]), d = __builtin_amdgcn_readfirstlane(t_rowptr[a + 1]) - lo;
  if (d <= 1) return;
  if (d > 256) {
    if (lane == 0) {
      for (int q = lo + 1; q < lo + d; ++q) {
        const int v = t_perm[q];
        int r = q - 1;
        while (r >= lo && t_perm[r] > v) {
          t_perm[r + 1] = t_perm[r];
          --r;
        }
        t_perm[r + 1] = v;
      }
    }
    return;
  }
  int x[4], rank[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int idx = lane + 64 * k;
    x[k] = idx < d ? t_perm[lo + idx] : 0x7fffffff;
    rank[k] = 0;
  }
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    if (64 * kk < d) {  // (wave-uniform)
      const int n = d - 64 * kk < 64 ? d - 64 * kk : 64;
      for (int m = 0; m < n; ++m) {
        const int y = __shfl(x[kk], m);
#pragma unroll
        for (int k = 0; k < 4; ++k) rank[k] += y < x[k] ? 1 : 0;
      }
    }
  }
  __builtin_amdgcn_wave_barrier();  // (every entry is in a register before the first one is written back)
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (lane + 64 * k < d) t_perm[lo + rank[k]] = x[k];
}
__global__ __launch_bounds__(256) void gt_sort_kernel(int64_t N, const int32_t* t_rowptr, int32_t* t_perm) {
  const int64_t a = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (a >= N) return;
  gt_sort_group(threadIdx.x & 63, a, t_rowptr, t_perm);
}
// hints[0..2] = first atom with edges, one past the last atom with edges, largest segment (0, 0, 0 without edges)
__global__ __launch_bounds__(256) void gt_hints_kernel(int64_t N, const int32_t* rowptr, int32_t* hints) {
  int* s = reinterpret_cast<int*>(aa_smem);  // [3][256]
  int first = int(N), last = 0, dmax = 0;
  for (int64_t a = threadIdx.x; a < N; a += 256) {
    const int d = rowptr[a + 1] - rowptr[a];
    if (d > 0) {
      first = first < int(a) ? first : int(a);
      last = int(a) + 1;
      dmax = dmax > d ? dmax : d;
    }
  }
  s[threadIdx.x] = first;
  s[256 + threadIdx.x] = last;
  s[512 + threadIdx.x] = dmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < 256; ++t) {
      first = first < s[t] ? first : s[t];
      last = last > s[256 + t] ? last : s[256 + t];
      dmax = dmax > s[512 + t] ? dmax : s[512 + t];
    }
    hints[0] = last > 0 ? first : 0;
    hints[1] = last;
    hints[2] = dmax;
  }
}

}  // namespace

extern "C" size_t aa_nl_workspace_bytes(int64_t num_atoms) {
  const size_t N = size_t(std::max<int64_t>(0, num_atoms)), NC = size_t(max_cells(num_atoms));
  return 2 * align_up(sizeof(int) * (NC + 1)) + 3 * align_up(sizeof(int) * N) + align_up(sizeof(int) * 3 * N) +
         align_up(sizeof(double) * 3 * N) + align_up(sizeof(int) * (N + 1)) +
         align_up(sizeof(int) * (std::max(N, NC) / kScanBlock + 2));
}

namespace {

constexpr size_t kTableBytes = sizeof(double) * kMaxTypes * kMaxTypes;

// what every entry point that takes an aa_nl_types checks; fills `rc2` [T*T] with min(r_cap, table)^2 (r_cap <= 0: the table alone)
// and `r_max` with the largest of min(r_cap, table)
int check_types(const aa_nl_types* t, int64_t num_atoms, double r_cap, const char* who, std::vector<double>& rc2, double& r_max) {
  const std::string w(who);
  AA_REQUIRE(t, w + ": null types");
  AA_REQUIRE(t->num_types >= 1 && t->num_types <= kMaxTypes, w + ": num_types must lie in [1, 64]");
  AA_REQUIRE(t->cutoffs, w + ": null cutoffs");
  AA_REQUIRE(t->atom_types || num_atoms == 0, w + ": null atom_types");
  const int TT = t->num_types * t->num_types;
  rc2.resize(size_t(TT));
  r_max = 0.0;
  for (int q = 0; q < TT; ++q) {
    const double c = t->cutoffs[q];
    AA_REQUIRE(std::isfinite(c) && c > 0.0, w + ": cutoffs must be positive and finite");
    const double r = r_cap > 0.0 ? std::min(r_cap, c) : c;
    rc2[size_t(q)] = r * r;
    r_max = std::max(r_max, r);
  }
  return AA_OK;
}

// typed workspace = the untyped one, then wtype [N], the squared table [64*64], the bad-type flag
int plan_nl_typed(const aa_nl_input* in, const aa_nl_types* types, void* ws, size_t ws_bytes, const char* who, NlDev& d, NlTypesDev& ty,
                  std::vector<double>& rc2) {
  AA_REQUIRE(in, std::string(who) + ": null argument");
  AA_REQUIRE(in->r_cut > 0.0, "aa_nl: r_cut must be positive");
  double r_list = 0.0;
  if (int rc = check_types(types, in->num_atoms, in->r_cut, who, rc2, r_list)) return rc;
  if (int rc = plan_nl(in, ws, ws_bytes, aa_nl_typed_workspace_bytes(in->num_atoms), r_list, d)) return rc;
  char* base = static_cast<char*>(ws) + aa_nl_workspace_bytes(in->num_atoms);
  ty.atom_types = types->atom_types;
  ty.wtype = reinterpret_cast<int*>(base);
  base += align_up(sizeof(int) * size_t(d.N));
  ty.rc2 = reinterpret_cast<const double*>(base);
  base += align_up(kTableBytes);
  ty.bad_type = reinterpret_cast<int*>(base);
  ty.T = types->num_types;
  return AA_OK;
}

// both list builds: `types` == nullptr is the untyped one
int nl_count(const aa_nl_input* in, const aa_nl_types* types, void* workspace, size_t workspace_bytes, int32_t* rowptr, int64_t* num_edges,
             aa_stream stream) {
  NlDev d{};
  NlTypesDev ty{};
  std::vector<double> rc2;
  const char* who = types ? "aa_nl_count_typed" : "aa_nl_count";
  if (types) {
    if (int rc = plan_nl_typed(in, types, workspace, workspace_bytes, who, d, ty, rc2)) return rc;
  } else {
    if (int rc = plan_nl(in, workspace, workspace_bytes, in ? aa_nl_workspace_bytes(in->num_atoms) : 0, in ? in->r_cut : 0.0, d)) return rc;
  }
  AA_REQUIRE(rowptr && num_edges, std::string(who) + ": null output");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = int((d.N + 255) / 256);
  const bool f32 = in->dtype == AA_F32;
  AA_CHECK_HIP(hipMemsetAsync(d.cell_count, 0, sizeof(int) * (size_t(d.ncells) + 1), s));
  if (types) {
    AA_CHECK_HIP(hipMemcpyAsync(const_cast<double*>(ty.rc2), rc2.data(), sizeof(double) * rc2.size(), hipMemcpyHostToDevice, s));
    AA_CHECK_HIP(hipMemsetAsync(ty.bad_type, 0, sizeof(int), s));
  }
  if (d.N > 0) {
    if (!types) {
      if (f32)
        hipLaunchKernelGGL(nl_bin_kernel<float>, dim3(nb), dim3(256), 0, s, d, ty);
      else
        hipLaunchKernelGGL(nl_bin_kernel<double>, dim3(nb), dim3(256), 0, s, d, ty);
    } else if (types->types_are_int64) {
      if (f32)
        hipLaunchKernelGGL((nl_bin_kernel<float, 2>), dim3(nb), dim3(256), 0, s, d, ty);
      else
        hipLaunchKernelGGL((nl_bin_kernel<double, 2>), dim3(nb), dim3(256), 0, s, d, ty);
    } else {
      if (f32)
        hipLaunchKernelGGL((nl_bin_kernel<float, 1>), dim3(nb), dim3(256), 0, s, d, ty);
      else
        hipLaunchKernelGGL((nl_bin_kernel<double, 1>), dim3(nb), dim3(256), 0, s, d, ty);
    }
  }
  launch_scan(d.cell_count, d.cell_start, int64_t(d.ncells), d.scan_tmp, s);
  if (d.N > 0) {
    hipLaunchKernelGGL(nl_cell_fill_kernel, dim3(nb), dim3(256), 0, s, d);
    hipLaunchKernelGGL(nl_cell_sort_kernel, dim3((d.ncells + 255) / 256), dim3(256), 0, s, d);
    if (types) {
      const size_t lds = sizeof(double) * size_t(ty.T) * size_t(ty.T);
      if (f32)
        hipLaunchKernelGGL((nl_pairs_kernel<float, false, true>), dim3(nb), dim3(256), lds, s, d, nullptr, nullptr, nullptr, nullptr, nullptr, ty);
      else
        hipLaunchKernelGGL((nl_pairs_kernel<double, false, true>), dim3(nb), dim3(256), lds, s, d, nullptr, nullptr, nullptr, nullptr, nullptr, ty);
    } else if (f32) {
      hipLaunchKernelGGL((nl_pairs_kernel<float, false>), dim3(nb), dim3(256), 0, s, d, nullptr, nullptr, nullptr, nullptr, nullptr, ty);
    } else {
      hipLaunchKernelGGL((nl_pairs_kernel<double, false>), dim3(nb), dim3(256), 0, s, d, nullptr, nullptr, nullptr, nullptr, nullptr, ty);
    }
  }
  launch_scan(d.counts, rowptr, d.N, d.scan_tmp, s);
  AA_CHECK_HIP(hipGetLastError());
  int32_t total = 0, bad = 0;
  AA_CHECK_HIP(hipMemcpyAsync(&total, rowptr + d.N, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (types) AA_CHECK_HIP(hipMemcpyAsync(&bad, ty.bad_type, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  AA_CHECK_HIP(hipStreamSynchronize(s));
  AA_REQUIRE(!bad, std::string(who) + ": atom_types outside [0, num_types)");
  AA_REQUIRE(total >= 0, std::string(who) + ": more than 2^31 edges");
  *num_edges = total;
  return AA_OK;
}

int nl_fill(const aa_nl_input* in, const aa_nl_types* types, void* workspace, size_t workspace_bytes, const int32_t* rowptr, int32_t* center,
            int32_t* nbr, int32_t* cell_shift, void* shift_vec, aa_stream stream) {
  NlDev d{};
  NlTypesDev ty{};
  std::vector<double> rc2;
  const char* who = types ? "aa_nl_fill_typed" : "aa_nl_fill";
  if (types) {
    if (int rc = plan_nl_typed(in, types, workspace, workspace_bytes, who, d, ty, rc2)) return rc;
  } else {
    if (int rc = plan_nl(in, workspace, workspace_bytes, in ? aa_nl_workspace_bytes(in->num_atoms) : 0, in ? in->r_cut : 0.0, d)) return rc;
  }
  AA_REQUIRE(rowptr && center && nbr, std::string(who) + ": null output");
  if (d.N == 0) return AA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = int((d.N + 255) / 256);
  if (types) {  // (wtype and the squared table are where the count call left them)
    const size_t lds = sizeof(double) * size_t(ty.T) * size_t(ty.T);
    if (in->dtype == AA_F32)
      hipLaunchKernelGGL((nl_pairs_kernel<float, true, true>), dim3(nb), dim3(256), lds, s, d, rowptr, center, nbr, cell_shift, shift_vec, ty);
    else
      hipLaunchKernelGGL((nl_pairs_kernel<double, true, true>), dim3(nb), dim3(256), lds, s, d, rowptr, center, nbr, cell_shift, shift_vec, ty);
  } else if (in->dtype == AA_F32) {
    hipLaunchKernelGGL((nl_pairs_kernel<float, true>), dim3(nb), dim3(256), 0, s, d, rowptr, center, nbr, cell_shift, shift_vec, ty);
  } else {
    hipLaunchKernelGGL((nl_pairs_kernel<double, true>), dim3(nb), dim3(256), 0, s, d, rowptr, center, nbr, cell_shift, shift_vec, ty);
  }
  AA_CHECK_HIP(hipGetLastError());
  return AA_OK;
}

}  // namespace

extern "C" size_t aa_nl_typed_workspace_bytes(int64_t num_atoms) {
  const size_t N = size_t(std::max<int64_t>(0, num_atoms));
  return aa_nl_workspace_bytes(num_atoms) + align_up(sizeof(int) * N) + align_up(kTableBytes) + align_up(sizeof(int));
}

extern "C" int aa_nl_count(const aa_nl_input* in, void* workspace, size_t workspace_bytes, int32_t* rowptr, int64_t* num_edges,
                           aa_stream stream) {
  return nl_count(in, nullptr, workspace, workspace_bytes, rowptr, num_edges, stream);
}

extern "C" int aa_nl_fill(const aa_nl_input* in, void* workspace, size_t workspace_bytes, const int32_t* rowptr, int32_t* center,
                          int32_t* nbr, int32_t* cell_shift, void* shift_vec, aa_stream stream) {
  return nl_fill(in, nullptr, workspace, workspace_bytes, rowptr, center, nbr, cell_shift, shift_vec, stream);
}

extern "C" int aa_nl_count_typed(const aa_nl_input* in, const aa_nl_types* types, void* workspace, size_t workspace_bytes, int32_t* rowptr,
                                 int64_t* num_edges, aa_stream stream) {
  AA_REQUIRE(types, "aa_nl_count_typed: null types");
  return nl_count(in, types, workspace, workspace_bytes, rowptr, num_edges, stream);
}

extern "C" int aa_nl_fill_typed(const aa_nl_input* in, const aa_nl_types* types, void* workspace, size_t workspace_bytes,
                                const int32_t* rowptr, int32_t* center, int32_t* nbr, int32_t* cell_shift, void* shift_vec,
                                aa_stream stream) {
  AA_REQUIRE(types, "aa_nl_fill_typed: null types");
  return nl_fill(in, types, workspace, workspace_bytes, rowptr, center, nbr, cell_shift, shift_vec, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// aa_nl_frames_*: the list of a batch of small frames, every frame in its own cell.  No cell grid: one wave per centre atom walks
// the atoms of its frame, 64 per pass, once per periodic image.  A listed pair's position is rowptr[centre] + its rank among the
// listed pairs of the segment: an inclusive prefix sum over the lanes plus the pairs of the earlier passes (the shuffle form of
// prune_kernel, which also runs in the CPU emulation build).  No atomic decides a position: images ascending, then neighbour id.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int kNoBadFrame = 0x7fffffff;
enum { FRAME_BAD_OFFSETS = 0, FRAME_BAD_SINGULAR = 1, FRAME_BAD_IMAGES = 2 };  // *bad = 4 * frame + reason of the FIRST refused frame

struct NlFramesDev {
  int64_t N;
  int B;
  const void* pos;
  const double* cells;         // [B,9] the caller's
  const int32_t* frame_atoms;  // [B+1] the caller's
  int pbc[3];
  double r_cut, rc2;
  // workspace
  double* inv;      // [B][9]
  int* kimg;        // [B][3]
  int* range;       // [B][2] the clamped atom range
  int* reason;      // [B] -1, or why the frame is refused
  int* atom_frame;  // [N] (-1: in no frame)
  int* wrap;        // [N][3]
  double* wpos;     // [N][3]
  int* counts;      // [N+1]
  int* scan_tmp;    // [N / 4096 + 2]
  int* bad;         // kNoBadFrame, or 4 * frame + reason
};

// one thread per frame
__global__ __launch_bounds__(256) void nlf_setup_kernel(NlFramesDev d) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= d.B) return;
  const int64_t f0 = d.frame_atoms[b], f1 = d.frame_atoms[b + 1];
  const int64_t lo = f0 < 0 ? 0 : (f0 > d.N ? d.N : f0);
  const int64_t hi = f1 < lo ? lo : (f1 > d.N ? d.N : f1);
  int reason = (lo != f0 || hi != f1) ? FRAME_BAD_OFFSETS : -1;
  const double* c = d.cells + 9 * int64_t(b);
  const double det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
  double inv[9];
  int k[3] = {0, 0, 0};
  if (!(fabs(det) > 1e-12)) {  // (a NaN lands here too)
    if (reason < 0) reason = FRAME_BAD_SINGULAR;
    for (int q = 0; q < 9; ++q) inv[q] = 0.0;
  } else {
    // inverse (pos = s @ cell  =>  s = pos @ inv), as plan_nl
    inv[0] = (c[4] * c[8] - c[5] * c[7]) / det;
    inv[1] = (c[2] * c[7] - c[1] * c[8]) / det;
    inv[2] = (c[1] * c[5] - c[2] * c[4]) / det;
    inv[3] = (c[5] * c[6] - c[3] * c[8]) / det;
    inv[4] = (c[0] * c[8] - c[2] * c[6]) / det;
    inv[5] = (c[2] * c[3] - c[0] * c[5]) / det;
    inv[6] = (c[3] * c[7] - c[4] * c[6]) / det;
    inv[7] = (c[1] * c[6] - c[0] * c[7]) / det;
    inv[8] = (c[0] * c[4] - c[1] * c[3]) / det;
    for (int a = 0; a < 3; ++a) {
      // perpendicular height along lattice direction a = 1 / |column a of inv|; wrapped atoms differ by less than one cell along a,
      // so an image |n| > r_cut / h cannot hold a pair
      const double n2 = inv[a] * inv[a] + inv[3 + a] * inv[3 + a] + inv[6 + a] * inv[6 + a];
      const double images = d.pbc[a] ? ceil(d.r_cut * sqrt(n2) - 1e-12) : 0.0;
      if (!(images <= 64.0)) {
        if (reason < 0) reason = FRAME_BAD_IMAGES;
      } else {
        k[a] = int(images);
      }
    }
  }
  if (reason >= 0) k[0] = k[1] = k[2] = 0;
  d.reason[b] = reason;
  for (int q = 0; q < 9; ++q) d.inv[9 * int64_t(b) + q] = inv[q];
  for (int a = 0; a < 3; ++a) d.kimg[3 * b + a] = k[a];
  d.range[2 * b] = int(lo);
  d.range[2 * b + 1] = int(hi);
  for (int64_t i = lo; i < hi; ++i) d.atom_frame[i] = b;
}

// one workgroup: the first refused frame, by a minimum over the frames (no atomic: the same answer on every call)
__global__ __launch_bounds__(256) void nlf_first_bad_kernel(NlFramesDev d) {
  int* sMin = reinterpret_cast<int*>(aa_smem);  // [256]
  int first = kNoBadFrame;
  for (int b = threadIdx.x; b < d.B; b += 256)
    if (d.reason[b] >= 0 && first == kNoBadFrame) first = 4 * b + d.reason[b];
  sMin[threadIdx.x] = first;
  __syncthreads();
  for (int st = 128; st >= 1; st >>= 1) {
    if (int(threadIdx.x) < st && sMin[threadIdx.x + st] < sMin[threadIdx.x]) sMin[threadIdx.x] = sMin[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) *d.bad = sMin[0];
}

// one thread per atom: the position wrapped into the cell of its frame along periodic directions (the arithmetic of nl_bin_kernel)
template <typename T>
__global__ __launch_bounds__(256) void nlf_wrap_kernel(NlFramesDev d) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= d.N) return;
  const T* p = static_cast<const T*>(d.pos) + 3 * i;
  const double x = double(p[0]), y = double(p[1]), z = double(p[2]);
  int f = d.atom_frame[i];
  f = f < 0 || f >= d.B ? -1 : f;
  int w[3] = {0, 0, 0};
  double cx = 0.0, cy = 0.0, cz = 0.0;
  if (f >= 0) {
    const double* inv = d.inv + 9 * int64_t(f);
    const double* c = d.cells + 9 * int64_t(f);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double s = x * inv[0 * 3 + a] + y * inv[1 * 3 + a] + z * inv[2 * 3 + a];
      if (d.pbc[a] && s == s && fabs(s) < 1e9) {  // (a position that is not a number, or absurdly far away, is left where it is)
        const double fl = floor(s);
        w[a] = -int(fl);
        s -= fl;
        if (s >= 1.0) w[a] -= 1;  // rounding: -1e-17 - floor(.) == 1.0
      }
    }
    cx = w[0] * c[0] + w[1] * c[3] + w[2] * c[6];
    cy = w[0] * c[1] + w[1] * c[4] + w[2] * c[7];
    cz = w[0] * c[2] + w[1] * c[5] + w[2] * c[8];
  }
  d.wpos[3 * i + 0] = x + cx;
  d.wpos[3 * i + 1] = y + cy;
  d.wpos[3 * i + 2] = z + cz;
  d.wrap[3 * i + 0] = w[0];
  d.wrap[3 * i + 1] = w[1];
  d.wrap[3 * i + 2] = w[2];
}

// One wave per centre atom, four per workgroup.  Count (FILL = false) and fill are the same code: the same predicate in the same
// double arithmetic, so rowptr always matches what fill writes.  After a count that raised the flag, fill writes nothing.
template <typename T, bool FILL>
__global__ __launch_bounds__(256) void nlf_pairs_kernel(NlFramesDev d, const int32_t* rowptr, int32_t* center, int32_t* nbr,
                                                        int32_t* cell_shift, void* shift_vec) {
  const int lane = threadIdx.x & 63;
  const int64_t i = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= d.N) return;  // (wave-uniform: every lane of a wave takes part in every exchange below)
  const bool refused = *d.bad != kNoBadFrame;
  int f = d.atom_frame[i];
  f = f < 0 || f >= d.B ? -1 : f;
  if (refused || f < 0) {
    if (!FILL && lane == 0) d.counts[i] = 0;
    return;
  }
  const int lo = d.range[2 * f], hi = d.range[2 * f + 1];
  const int k0 = d.kimg[3 * f], k1 = d.kimg[3 * f + 1], k2 = d.kimg[3 * f + 2];
  const double* c = d.cells + 9 * int64_t(f);
  const double xi = d.wpos[3 * i], yi = d.wpos[3 * i + 1], zi = d.wpos[3 * i + 2];
  const int wi0 = d.wrap[3 * i], wi1 = d.wrap[3 * i + 1], wi2 = d.wrap[3 * i + 2];
  int64_t o = FILL ? rowptr[i] : 0;  // where this pass's first pair goes
  int cnt = 0;
  for (int n0 = -k0; n0 <= k0; ++n0)
    for (int n1 = -k1; n1 <= k1; ++n1)
      for (int n2 = -k2; n2 <= k2; ++n2) {
        const double sx = n0 * c[0] + n1 * c[3] + n2 * c[6];
        const double sy = n0 * c[1] + n1 * c[4] + n2 * c[7];
        const double sz = n0 * c[2] + n1 * c[5] + n2 * c[8];
        const bool home = n0 == 0 && n1 == 0 && n2 == 0;
        for (int j0 = lo; j0 < hi; j0 += 64) {
          const int j = j0 + lane;
          bool listed = j < hi && !(home && j == i);
          if (listed) {
            const double dx = d.wpos[3 * int64_t(j)] + sx - xi, dy = d.wpos[3 * int64_t(j) + 1] + sy - yi,
                         dz = d.wpos[3 * int64_t(j) + 2] + sz - zi;
            listed = dx * dx + dy * dy + dz * dz < d.rc2;
          }
          if constexpr (FILL) {
            int x = listed ? 1 : 0;
            for (int st = 1; st < 64; st <<= 1) {
              const int y = __shfl_up(x, st);
              if (lane >= st) x += y;
            }
            if (listed) {
              const int64_t e = o + x - 1;
              center[e] = int32_t(i);
              nbr[e] = j;
              // undo the wrapping: r_e = pos[j] - pos[i] + S @ cell with S = n + w_j - w_i
              const int S0 = n0 + d.wrap[3 * int64_t(j)] - wi0, S1 = n1 + d.wrap[3 * int64_t(j) + 1] - wi1,
                        S2 = n2 + d.wrap[3 * int64_t(j) + 2] - wi2;
              if (cell_shift) {
                cell_shift[3 * e] = S0;
                cell_shift[3 * e + 1] = S1;
                cell_shift[3 * e + 2] = S2;
              }
              if (shift_vec) {
                T* sv = static_cast<T*>(shift_vec) + 3 * e;
                sv[0] = T(S0 * c[0] + S1 * c[3] + S2 * c[6]);
                sv[1] = T(S0 * c[1] + S1 * c[4] + S2 * c[7]);
                sv[2] = T(S0 * c[2] + S1 * c[5] + S2 * c[8]);
              }
            }
            o += __shfl(x, 63);
          } else {
            cnt += listed ? 1 : 0;
          }
        }
      }
  if constexpr (!FILL) {
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    if (lane == 0) d.counts[i] = cnt;
  }
}

int plan_nl_frames(const aa_nl_frames_input* in, const aa_frames* frames, void* ws, size_t ws_bytes, const char* who, NlFramesDev& d) {
  const std::string w(who);
  AA_REQUIRE(in && frames && ws, w + ": null argument");
  AA_REQUIRE(in->num_atoms >= 0 && in->num_atoms < (int64_t(1) << 31), w + ": atom count out of range");
  AA_REQUIRE(frames->num_frames >= 0 && frames->num_frames < (1 << 29), w + ": num_frames out of range");
  AA_REQUIRE(in->dtype == AA_F32 || in->dtype == AA_F64, w + ": bad dtype");
  AA_REQUIRE(in->r_cut > 0.0 && std::isfinite(in->r_cut), w + ": r_cut must be positive and finite");
  AA_REQUIRE(in->pos || in->num_atoms == 0, w + ": null positions");
  AA_REQUIRE((frames->frame_atoms && in->cells) || frames->num_frames == 0, w + ": null frame_atoms or cells");
  if (ws_bytes < aa_nl_frames_workspace_bytes(in->num_atoms, frames->num_frames)) return fail(AA_ERR_WORKSPACE, w + ": workspace too small");
  d.N = in->num_atoms;
  d.B = frames->num_frames;
  d.pos = in->pos;
  d.cells = in->cells;
  d.frame_atoms = frames->frame_atoms;
  for (int a = 0; a < 3; ++a) d.pbc[a] = in->pbc[a] ? 1 : 0;
  d.r_cut = in->r_cut;
  d.rc2 = in->r_cut * in->r_cut;
  char* base = static_cast<char*>(ws);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* r = base + o;
    o += align_up(bytes);
    return r;
  };
  const size_t N = size_t(d.N), B = size_t(d.B);
  d.inv = reinterpret_cast<double*>(take(sizeof(double) * 9 * B));
  d.wpos = reinterpret_cast<double*>(take(sizeof(double) * 3 * N));
  d.kimg = reinterpret_cast<int*>(take(sizeof(int) * 3 * B));
  d.range = reinterpret_cast<int*>(take(sizeof(int) * 2 * B));
  d.reason = reinterpret_cast<int*>(take(sizeof(int) * B));
  d.atom_frame = reinterpret_cast<int*>(take(sizeof(int) * N));
  d.wrap = reinterpret_cast<int*>(take(sizeof(int) * 3 * N));
  d.counts = reinterpret_cast<int*>(take(sizeof(int) * (N + 1)));
  d.scan_tmp = reinterpret_cast<int*>(take(sizeof(int) * (N / kScanBlock + 2)));
  d.bad = reinterpret_cast<int*>(take(sizeof(int)));
  return AA_OK;
}

}  // namespace

extern "C" size_t aa_nl_frames_workspace_bytes(int64_t num_atoms, int32_t num_frames) {
  const size_t N = size_t(std::max<int64_t>(0, num_atoms)), B = size_t(std::max<int32_t>(0, num_frames));
  return align_up(sizeof(double) * 9 * B) + align_up(sizeof(double) * 3 * N) + align_up(sizeof(int) * 3 * B) + align_up(sizeof(int) * 2 * B) +
         align_up(sizeof(int) * B) + align_up(sizeof(int) * N) + align_up(sizeof(int) * 3 * N) + align_up(sizeof(int) * (N + 1)) +
         align_up(sizeof(int) * (N / kScanBlock + 2)) + align_up(sizeof(int));
}

extern "C" int aa_nl_frames_count(const aa_nl_frames_input* in, const aa_frames* frames, void* workspace, size_t workspace_bytes,
                                  int32_t* rowptr, int64_t* num_edges, aa_stream stream) {
  NlFramesDev d{};
  if (int rc = plan_nl_frames(in, frames, workspace, workspace_bytes, "aa_nl_frames_count", d)) return rc;
  AA_REQUIRE(rowptr && num_edges, "aa_nl_frames_count: null output");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d.N > 0) AA_CHECK_HIP(hipMemsetAsync(d.atom_frame, 0xff, sizeof(int) * size_t(d.N), s));  // -1: in no frame
  if (d.B > 0) hipLaunchKernelGGL(nlf_setup_kernel, dim3((d.B + 255) / 256), dim3(256), 0, s, d);
  hipLaunchKernelGGL(nlf_first_bad_kernel, dim3(1), dim3(256), sizeof(int) * 256, s, d);
  if (d.N > 0) {
    const dim3 atoms((unsigned)((d.N + 255) / 256)), waves((unsigned)((d.N + 3) / 4));
    if (in->dtype == AA_F32) {
      hipLaunchKernelGGL(nlf_wrap_kernel<float>, atoms, dim3(256), 0, s, d);
      hipLaunchKernelGGL((nlf_pairs_kernel<float, false>), waves, dim3(256), 0, s, d, nullptr, nullptr, nullptr, nullptr, nullptr);
    } else {
      hipLaunchKernelGGL(nlf_wrap_kernel<double>, atoms, dim3(256), 0, s, d);
      hipLaunchKernelGGL((nlf_pairs_kernel<double, false>), waves, dim3(256), 0, s, d, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
  }
  launch_scan(d.counts, rowptr, d.N, d.scan_tmp, s);
  AA_CHECK_HIP(hipGetLastError());
  int32_t total = 0, bad = kNoBadFrame;
  AA_CHECK_HIP(hipMemcpyAsync(&total, rowptr + d.N, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  AA_CHECK_HIP(hipMemcpyAsync(&bad, d.bad, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  AA_CHECK_HIP(hipStreamSynchronize(s));
  if (bad != kNoBadFrame) {
    static const char* const why[] = {"frame_atoms outside [0, num_atoms] or decreasing", "singular cell",
                                      "cell much smaller than r_cut (more than 64 images along one direction)", "?"};
    return fail(AA_ERR_INVALID, "aa_nl_frames_count: frame " + std::to_string(bad / 4) + ": " + why[bad % 4]);
  }
  AA_REQUIRE(total >= 0, "aa_nl_frames_count: more than 2^31 edges");
  *num_edges = total;
  return AA_OK;
}

extern "C" int aa_nl_frames_fill(const aa_nl_frames_input* in, const aa_frames* frames, void* workspace, size_t workspace_bytes,
                                 const int32_t* rowptr, int32_t* center, int32_t* nbr, int32_t* cell_shift, void* shift_vec, aa_stream stream) {
  NlFramesDev d{};
  if (int rc = plan_nl_frames(in, frames, workspace, workspace_bytes, "aa_nl_frames_fill", d)) return rc;
  AA_REQUIRE(rowptr && center && nbr, "aa_nl_frames_fill: null output");
  if (d.N == 0 || d.B == 0) return AA_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 waves((unsigned)((d.N + 3) / 4));
  if (in->dtype == AA_F32)
    hipLaunchKernelGGL((nlf_pairs_kernel<float, true>), waves, dim3(256), 0, s, d, rowptr, center, nbr, cell_shift, shift_vec);
  else
    hipLaunchKernelGGL((nlf_pairs_kernel<double, true>), waves, dim3(256), 0, s, d, rowptr, center, nbr, cell_shift, shift_vec);
  AA_CHECK_HIP(hipGetLastError());
  return AA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// aa_graph_prune_*: stable compaction of a center-sorted list somebody else built, by per-type-pair cutoffs.
// ONE WAVE PER CENTER SEGMENT (four per workgroup), 64 edges per pass: the lanes read nbr / shift_vec of consecutive edges, so
// these streams are coalesced, which a thread-per-atom loop (the form of nl_pairs_kernel, whose inner loop walks cells, not a
// contiguous array) would not give; at the segment lengths of these lists (~10-130 edges) a wave is one to three passes per
// center.  A surviving edge's position is out_rowptr[center] + its rank among the survivors of its segment: the rank is an
// inclusive prefix sum over the lanes (six __shfl_up steps per pass; a ballot + popcount gives the same number -- the shuffle
// form is the one that also runs in the CPU emulation build the tests use) plus the survivors of the earlier passes.  No atomic
// decides a position.  Count and fill call the same prune_keeps().  The table is read from global memory (<= 32 KB, one cached
// load per edge next to the pos[nbr] and type gathers).  Neither form was timed against the other.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct PruneDev {
  int64_t N, E;
  const void* pos;
  const int32_t* rowptr;
  const int32_t* nbr;
  const void* shift_vec;
  const void* atom_types;
  const double* rc2;  // [T,T] workspace: table^2
  int* bad_type;      // workspace
  int* counts;        // [N+1] workspace
  int T;
};

// (a neighbour id outside [0, N) -- a malformed list -- is dropped by both passes alike, nothing is read out of bounds)
template <typename T, typename TT>
__device__ __forceinline__ bool prune_keeps(const PruneDev& p, int64_t e, int j, double xi, double yi, double zi, const double* row) {
  if (j < 0 || j >= p.N) return false;
  const T* pj = static_cast<const T*>(p.pos) + 3 * int64_t(j);
  double dx = double(pj[0]) - xi, dy = double(pj[1]) - yi, dz = double(pj[2]) - zi;
  if (p.shift_vec) {
    const T* sv = static_cast<const T*>(p.shift_vec) + 3 * e;
    dx += double(sv[0]);
    dy += double(sv[1]);
    dz += double(sv[2]);
  }
  return dx * dx + dy * dy + dz * dz < row[clamped_type<TT>(p.atom_types, j, p.T, p.bad_type)];
}

template <typename T, typename TT, bool FILL>
__global__ __launch_bounds__(256) void prune_kernel(PruneDev p, const int32_t* out_rowptr, int32_t* out_center, int32_t* out_nbr,
                                                    void* out_shift_vec, int32_t* kept) {
  const int lane = threadIdx.x & 63;
  const int64_t a = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (a >= p.N) return;  // (wave-uniform: every lane of a wave takes part in every exchange below)
  int64_t lo = p.rowptr[a], hi = p.rowptr[a + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > p.E ? p.E : hi;  // (row pointers beyond the list -- malformed -- read nothing)
  if (hi <= lo) {
    if (!FILL && lane == 0) p.counts[a] = 0;
    return;
  }
  const T* pi = static_cast<const T*>(p.pos) + 3 * a;
  const double xi = double(pi[0]), yi = double(pi[1]), zi = double(pi[2]);
  const double* row = p.rc2 + clamped_type<TT>(p.atom_types, a, p.T, p.bad_type) * p.T;
  int64_t o = FILL ? out_rowptr[a] : 0;  // where this pass's first survivor goes
  int cnt = 0;
  for (int64_t e0 = lo; e0 < hi; e0 += 64) {
    const int64_t e = e0 + lane;
    const int j = e < hi ? p.nbr[e] : -1;
    const bool keep = e < hi && prune_keeps<T, TT>(p, e, j, xi, yi, zi, row);
    if constexpr (FILL) {
      int x = keep ? 1 : 0;
      for (int st = 1; st < 64; st <<= 1) {
        const int y = __shfl_up(x, st);
        if (lane >= st) x += y;
      }
      if (keep) {
        const int64_t q = o + x - 1;
        out_center[q] = int32_t(a);
        out_nbr[q] = j;
        if (kept) kept[q] = int32_t(e);
        if (out_shift_vec) {
          T* dst = static_cast<T*>(out_shift_vec) + 3 * q;
          if (p.shift_vec) {
            const T* sv = static_cast<const T*>(p.shift_vec) + 3 * e;
            dst[0] = sv[0];
            dst[1] = sv[1];
            dst[2] = sv[2];
          } else {
            dst[0] = dst[1] = dst[2] = T(0);
          }
        }
      }
      o += __shfl(x, 63);
    } else {
      cnt += keep ? 1 : 0;
    }
  }
  if constexpr (!FILL) {
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    if (lane == 0) p.counts[a] = cnt;
  }
}

// workspace: counts [N+1], scan scratch, the squared table [64*64], the bad-type flag
int plan_prune(const aa_prune_input* in, const aa_nl_types* types, void* ws, size_t ws_bytes, const char* who, PruneDev& p,
               std::vector<double>& rc2, int** scan_tmp) {
  const std::string w(who);
  AA_REQUIRE(in && ws, w + ": null argument");
  AA_REQUIRE(in->num_atoms >= 0 && in->num_atoms < (int64_t(1) << 31) && in->num_edges >= 0 && in->num_edges < (int64_t(1) << 31),
             w + ": size out of range");
  AA_REQUIRE(in->dtype == AA_F32 || in->dtype == AA_F64, w + ": bad dtype");
  AA_REQUIRE(in->rowptr && (in->pos || in->num_atoms == 0) && (in->nbr || in->num_edges == 0), w + ": null pos, rowptr or nbr");
  double r_max = 0.0;
  if (int rc = check_types(types, in->num_atoms, 0.0, who, rc2, r_max)) return rc;
  if (ws_bytes < aa_graph_prune_workspace_bytes(in->num_atoms)) return fail(AA_ERR_WORKSPACE, w + ": workspace too small");
  const size_t N = size_t(in->num_atoms);
  char* base = static_cast<char*>(ws);
  p.N = in->num_atoms;
  p.E = in->num_edges;
  p.pos = in->pos;
  p.rowptr = in->rowptr;
  p.nbr = in->nbr;
  p.shift_vec = in->shift_vec;
  p.atom_types = types->atom_types;
  p.T = types->num_types;
  p.counts = reinterpret_cast<int*>(base);
  base += align_up(sizeof(int) * (N + 1));
  *scan_tmp = reinterpret_cast<int*>(base);
  base += align_up(sizeof(int) * (N / kScanBlock + 2));
  p.rc2 = reinterpret_cast<const double*>(base);
  base += align_up(kTableBytes);
  p.bad_type = reinterpret_cast<int*>(base);
  return AA_OK;
}

template <bool FILL>
void launch_prune(const PruneDev& p, int dtype, bool types64, const int32_t* out_rowptr, int32_t* out_center, int32_t* out_nbr,
                  void* out_shift_vec, int32_t* kept, hipStream_t s) {
  const dim3 grid((unsigned)((p.N + 3) / 4)), block(256);
  if (dtype == AA_F32) {
    if (types64)
      hipLaunchKernelGGL((prune_kernel<float, int64_t, FILL>), grid, block, 0, s, p, out_rowptr, out_center, out_nbr, out_shift_vec, kept);
    else
      hipLaunchKernelGGL((prune_kernel<float, int32_t, FILL>), grid, block, 0, s, p, out_rowptr, out_center, out_nbr, out_shift_vec, kept);
  } else {
    if (types64)
      hipLaunchKernelGGL((prune_kernel<double, int64_t, FILL>), grid, block, 0, s, p, out_rowptr, out_center, out_nbr, out_shift_vec, kept);
    else
      hipLaunchKernelGGL((prune_kernel<double, int32_t, FILL>), grid, block, 0, s, p, out_rowptr, out_center, out_nbr, out_shift_vec, kept);
  }
}

}  // namespace

extern "C" size_t aa_graph_prune_workspace_bytes(int64_t num_atoms) {
  const size_t N = size_t(std::max<int64_t>(0, num_atoms));
  return align_up(sizeof(int) * (N + 1)) + align_up(sizeof(int) * (N / kScanBlock + 2)) + align_up(kTableBytes) + align_up(sizeof(int));
}

extern "C" int aa_graph_prune_count(const aa_prune_input* in, const aa_nl_types* types, void* workspace, size_t workspace_bytes,
                                    int32_t* out_rowptr, int64_t* out_num_edges, aa_stream stream) {
  PruneDev p{};
  std::vector<double> rc2;
  int* scan_tmp = nullptr;
  if (int rc = plan_prune(in, types, workspace, workspace_bytes, "aa_graph_prune_count", p, rc2, &scan_tmp)) return rc;
  AA_REQUIRE(out_rowptr && out_num_edges, "aa_graph_prune_count: null output");
  hipStream_t s = static_cast<hipStream_t>(stream);
  AA_CHECK_HIP(hipMemcpyAsync(const_cast<double*>(p.rc2), rc2.data(), sizeof(double) * rc2.size(), hipMemcpyHostToDevice, s));
  AA_CHECK_HIP(hipMemsetAsync(p.bad_type, 0, sizeof(int), s));
  if (p.N > 0) launch_prune<false>(p, in->dtype, types->types_are_int64 != 0, nullptr, nullptr, nullptr, nullptr, nullptr, s);
  launch_scan(p.counts, out_rowptr, p.N, scan_tmp, s);
  AA_CHECK_HIP(hipGetLastError());
  int32_t total = 0, bad = 0;
  AA_CHECK_HIP(hipMemcpyAsync(&total, out_rowptr + p.N, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  AA_CHECK_HIP(hipMemcpyAsync(&bad, p.bad_type, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  AA_CHECK_HIP(hipStreamSynchronize(s));
  AA_REQUIRE(!bad, "aa_graph_prune_count: atom_types outside [0, num_types)");
  *out_num_edges = total;
  return AA_OK;
}

extern "C" int aa_graph_prune_fill(const aa_prune_input* in, const aa_nl_types* types, void* workspace, size_t workspace_bytes,
                                   const int32_t* out_rowptr, int32_t* out_center, int32_t* out_nbr, void* out_shift_vec, int32_t* kept,
                                   aa_stream stream) {
  PruneDev p{};
  std::vector<double> rc2;
  int* scan_tmp = nullptr;
  if (int rc = plan_prune(in, types, workspace, workspace_bytes, "aa_graph_prune_fill", p, rc2, &scan_tmp)) return rc;
  AA_REQUIRE(out_rowptr && out_center && out_nbr, "aa_graph_prune_fill: null output");
  if (p.N == 0 || p.E == 0) return AA_OK;
  // (the squared table is where the count call left it)
  launch_prune<true>(p, in->dtype, types->types_are_int64 != 0, out_rowptr, out_center, out_nbr, out_shift_vec, kept, static_cast<hipStream_t>(stream));
  AA_CHECK_HIP(hipGetLastError());
  return AA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// content fingerprint of a neighbour list (aa_graph_fingerprint): lets a host that caches graph structure by tensor
// IDENTITY (csrc/torch_ops.cpp) notice that the contents behind an unchanged tensor were rewritten through a raw pointer
// ---------------------------------------------------------------------------------------------------------------------
extern "C" size_t aa_graph_transpose_workspace_bytes(int64_t num_atoms) {
  const size_t N = size_t(std::max<int64_t>(0, num_atoms));
  return 2 * align_up(sizeof(int) * (N + 1)) + align_up(sizeof(int) * (N / kScanBlock + 2));
}

extern "C" int aa_graph_transpose(int64_t num_atoms, int64_t num_edges, const int32_t* rowptr, const int32_t* nbr, int32_t* t_rowptr,
                                  int32_t* t_perm, int32_t* hints3, void* workspace, size_t workspace_bytes, aa_stream stream) {
  AA_REQUIRE(num_atoms >= 0 && num_edges >= 0 && num_edges < (int64_t(1) << 31) && num_atoms < (int64_t(1) << 31), "aa_graph_transpose: size out of range");
  AA_REQUIRE(t_rowptr && (num_edges == 0 || (nbr && t_perm)) && workspace, "aa_graph_transpose: null argument");
  AA_REQUIRE(workspace_bytes >= aa_graph_transpose_workspace_bytes(num_atoms), "aa_graph_transpose: workspace too small");
  AA_REQUIRE(!hints3 || rowptr, "aa_graph_transpose: the hints need the row pointers");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t N = num_atoms, E = num_edges;
  char* w = static_cast<char*>(workspace);
  int* cnt = reinterpret_cast<int*>(w);
  int* cursor = reinterpret_cast<int*>(w + align_up(sizeof(int) * (N + 1)));
  int* scan_tmp = reinterpret_cast<int*>(w + 2 * align_up(sizeof(int) * (N + 1)));
  AA_CHECK_HIP(hipMemsetAsync(w, 0, 2 * align_up(sizeof(int) * (N + 1)), s));
  if (E > 0) hipLaunchKernelGGL(gt_count_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, nbr, E, N, cnt);
  launch_scan(cnt, t_rowptr, N, scan_tmp, s);
  if (E > 0) {
    hipLaunchKernelGGL(gt_place_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, nbr, E, N, t_rowptr, cursor, t_perm);
    hipLaunchKernelGGL(gt_sort_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, N, t_rowptr, t_perm);
  }
  if (hints3) hipLaunchKernelGGL(gt_hints_kernel, dim3(1), dim3(256), 3 * 256 * sizeof(int), s, N, rowptr, hints3);
  AA_CHECK_HIP(hipGetLastError());
  return AA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// aa_graph_build_*: the aa_graph of the list a host actually has -- edge_index [2,E], int64 or int32, rows a stride apart, edges
// in ANY order -- optionally reduced to the per-type-pair cutoffs on the way: center-sorted int32 CSR in stable order (ascending
// input edge id inside a segment), perm, shift vectors, the transposed CSR and the three hints.
//   count  one thread per input edge reads its center and neighbour (consecutive lanes, consecutive 8- or 4-byte elements: one
//          coalesced stream per row), raises the range flags and the sortedness flag (center[e-1] > center[e]; the line is the
//          lane's own or its neighbour's), evaluates prune_keeps -- the predicate of aa_graph_prune_*, the same function -- and
//          adds to the center histogram.  Lanes that hold the same center in a row (all of them in a sorted list) merge into ONE
//          integer atomic per run: the run length comes from six shuffle-doubling steps.  Counts do not depend on arrival order.
//          Then nl_scan_* -> out_rowptr, gt_hints_kernel -> hints, and with `types` a scan of the keep flags over the edges.
//   fill   reads the flags on the device (no host read).  Sorted input: output position = prefix sum of the keep flags (= e
//          without `types`), the edge is emitted where it stands.  Unsorted input: counting-sort placement by an atomic cursor,
//          then every center segment is RANKED by gt_sort_group (the code of gt_sort_kernel, serial branch beyond 256 entries),
//          so no atomic decides a final position; a gather pass then emits center / nbr / shift_vec / perm through perm.  The
//          emit also counts the neighbour histogram; nl_scan_* + a placement pass + gt_sort_kernel give t_rowptr / t_perm.
// A raised range flag makes every fill kernel return before it touches an output.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

enum { kResUnsorted = 0, kResBadCenter = 1, kResBadNbr = 2, kResBadType = 3, kResHints = 4, kResInts = 16 };

struct BuildDev {
  int64_t N, E, stride;
  const void* rows;       // edge_index: centers at [0, E), neighbours at [stride, stride + E)
  const void* shift_vec;  // [E,3] in input order, or nullptr
  int* a0;                // [N+1] workspace: center histogram (count), placement cursor (fill)
  int* a1;                // [N+1] workspace: neighbour histogram
  int* a2;                // [N+1] workspace: placement cursor of the transposition
  int* scan_tmp;          // [max(N, E) / 4096 + 2]
  int* res;               // [16] flags (0 unsorted, 1 / 2 bad center / neighbour: edge id + 1, 3 bad type) and hints [4..6]
  int* permw;             // [E] input ids in output order while they are ranked: the caller's perm, or workspace
  int* keepf;             // [E] workspace, typed only: 1 = the edge is kept
  int* kpos;              // [E+1] workspace, typed only: exclusive prefix sums of keepf
  PruneDev p;             // what prune_keeps reads: N, pos, shift_vec, atom_types, T, rc2, bad_type
};
struct BuildOut {
  int32_t *center, *nbr, *perm;
  void* shift_vec;
  int transposed;
};

template <typename IT, typename T, typename TT, bool TYPED>
__global__ __launch_bounds__(256) void gb_count_kernel(BuildDev b) {
  const int lane = threadIdx.x & 63;
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  int key = -1;  // the center this lane counts for; -1: nothing (every lane takes part in the exchanges below)
  if (e < b.E) {
    const IT* r0 = static_cast<const IT*>(b.rows);
    const int64_t c = int64_t(r0[e]), j = int64_t(r0[b.stride + e]);
    if (e > 0 && int64_t(r0[e - 1]) > c) b.res[kResUnsorted] = 1;
    const bool okc = c >= 0 && c < b.N, okj = j >= 0 && j < b.N;
    if (!okc) b.res[kResBadCenter] = int(e) + 1;
    if (!okj) b.res[kResBadNbr] = int(e) + 1;
    bool keep = okc && okj;
    if constexpr (TYPED) {
      if (keep) {
        const T* pi = static_cast<const T*>(b.p.pos) + 3 * c;
        const double* row = b.p.rc2 + clamped_type<TT>(b.p.atom_types, c, b.p.T, b.p.bad_type) * b.p.T;
        keep = prune_keeps<T, TT>(b.p, e, int(j), double(pi[0]), double(pi[1]), double(pi[2]), row);
      }
      b.keepf[e] = keep ? 1 : 0;
    }
    if (keep) key = int(c);
  }
  // len = how many lanes from this one on hold the same key without a gap, min(run, 2 st) after the step of width st
  int len = 1;
  for (int st = 1; st < 64; st <<= 1) {
    const int okey = __shfl_down(key, st), olen = __shfl_down(len, st);
    if (len == st && lane + st < 64 && okey == key) len += olen;
  }
  const int prev = __shfl_up(key, 1);
  if (key >= 0 && (lane == 0 || prev != key)) atomicAdd(&b.a0[key], len);
}

// W: a shift-vector component as a word of the dtype's size (copied, never computed with)
template <typename W>
__device__ __forceinline__ void gb_emit(const BuildDev& b, const BuildOut& o, int64_t q, int64_t e, int c, int j) {
  o.center[q] = c;
  o.nbr[q] = j;
  if (o.perm) o.perm[q] = int32_t(e);
  if (o.shift_vec) {
    W* dst = static_cast<W*>(o.shift_vec) + 3 * q;
    if (b.shift_vec) {
      const W* sv = static_cast<const W*>(b.shift_vec) + 3 * e;
      dst[0] = sv[0];
      dst[1] = sv[1];
      dst[2] = sv[2];
    } else {
      dst[0] = dst[1] = dst[2] = W(0);
    }
  }
  if (o.transposed) atomicAdd(&b.a1[j], 1);
}

template <typename IT, typename W, bool TYPED>
__global__ __launch_bounds__(256) void gb_place_kernel(BuildDev b, const int32_t* rowptr, BuildOut o) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= b.E || (b.res[kResBadCenter] | b.res[kResBadNbr])) return;
  if constexpr (TYPED) {
    if (!b.keepf[e]) return;
  }
  const IT* r0 = static_cast<const IT*>(b.rows);
  const int c = int(r0[e]);
  if (b.res[kResUnsorted]) {  // a slot of the segment, in arrival order: gb_sort_kernel ranks the segment afterwards
    b.permw[rowptr[c] + atomicAdd(&b.a0[c], 1)] = int(e);
    return;
  }
  int64_t q = e;
  if constexpr (TYPED) q = b.kpos[e];
  gb_emit<W>(b, o, q, e, c, int(r0[b.stride + e]));
}

__global__ __launch_bounds__(256) void gb_sort_kernel(BuildDev b, const int32_t* rowptr) {
  const int64_t a = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (a >= b.N || !b.res[kResUnsorted] || (b.res[kResBadCenter] | b.res[kResBadNbr])) return;  // (wave-uniform)
  gt_sort_group(threadIdx.x & 63, a, rowptr, b.permw);
}

template <typename IT, typename W>
__global__ __launch_bounds__(256) void gb_gather_kernel(BuildDev b, const int32_t* rowptr, BuildOut o) {
  const int64_t q = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (!b.res[kResUnsorted] || (b.res[kResBadCenter] | b.res[kResBadNbr]) || q >= rowptr[b.N]) return;
  const IT* r0 = static_cast<const IT*>(b.rows);
  const int64_t e = b.permw[q];
  gb_emit<W>(b, o, q, e, int(r0[e]), int(r0[b.stride + e]));
}

// gt_place_kernel for a list whose length the host does not know (rowptr[N], on the device)
__global__ __launch_bounds__(256) void gb_tplace_kernel(BuildDev b, const int32_t* rowptr, const int32_t* nbr, const int32_t* t_rowptr,
                                                        int32_t* t_perm) {
  const int64_t q = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if ((b.res[kResBadCenter] | b.res[kResBadNbr]) || q >= rowptr[b.N]) return;
  const int j = nbr[q];
  t_perm[t_rowptr[j] + atomicAdd(&b.a2[j], 1)] = int32_t(q);
}

size_t build_scan_ints(size_t N, size_t E) { return std::max(N, E) / kScanBlock + 2; }

int plan_build(const aa_edge_list* in, const aa_nl_types* types, void* ws, size_t ws_bytes, const char* who, BuildDev& b) {
  const std::string w(who);
  AA_REQUIRE(in, w + ": null argument");
  AA_REQUIRE(in->num_atoms >= 0 && in->num_atoms < (int64_t(1) << 31) && in->num_edges >= 0 && in->num_edges < (int64_t(1) << 31),
             w + ": size out of range (num_atoms and num_edges must lie in [0, 2^31))");
  AA_REQUIRE(ws, w + ": null workspace");
  AA_REQUIRE(in->index_is_int64 == 0 || in->index_is_int64 == 1, w + ": index_is_int64 must be 0 or 1");
  AA_REQUIRE(in->edge_index || in->num_edges == 0, w + ": null edge_index");
  AA_REQUIRE(in->row_stride >= in->num_edges, w + ": row_stride smaller than num_edges (the rows would overlap)");
  if (types || in->shift_vec) AA_REQUIRE(in->dtype == AA_F32 || in->dtype == AA_F64, w + ": bad dtype");
  AA_REQUIRE(!types || in->pos || in->num_atoms == 0, w + ": per-type-pair cutoffs need positions (null pos)");
  if (ws_bytes < aa_graph_build_workspace_bytes(in->num_atoms, in->num_edges)) return fail(AA_ERR_WORKSPACE, w + ": workspace too small");
  const size_t N = size_t(in->num_atoms), E = size_t(in->num_edges);
  char* base = static_cast<char*>(ws);
  auto take = [&](size_t bytes) {
    char* r = base;
    base += align_up(bytes);
    return r;
  };
  b.N = in->num_atoms;
  b.E = in->num_edges;
  b.stride = in->row_stride;
  b.rows = in->edge_index;
  b.shift_vec = in->shift_vec;
  b.a0 = reinterpret_cast<int*>(take(sizeof(int) * (N + 1)));
  b.a1 = reinterpret_cast<int*>(take(sizeof(int) * (N + 1)));
  b.a2 = reinterpret_cast<int*>(take(sizeof(int) * (N + 1)));
  b.scan_tmp = reinterpret_cast<int*>(take(sizeof(int) * build_scan_ints(N, E)));
  b.p.rc2 = reinterpret_cast<const double*>(take(kTableBytes));
  b.res = reinterpret_cast<int*>(take(sizeof(int) * kResInts));
  b.permw = reinterpret_cast<int*>(take(sizeof(int) * E));
  b.keepf = reinterpret_cast<int*>(take(sizeof(int) * E));
  b.kpos = reinterpret_cast<int*>(take(sizeof(int) * (E + 1)));
  b.p.N = b.N;
  b.p.E = b.E;
  b.p.pos = in->pos;
  b.p.shift_vec = in->shift_vec;
  b.p.bad_type = b.res + kResBadType;
  if (types) {
    b.p.atom_types = types->atom_types;
    b.p.T = types->num_types;
  }
  return AA_OK;
}

template <typename IT>
void launch_build_count(const BuildDev& b, const aa_nl_types* types, int dtype, dim3 grid, hipStream_t s) {
  if (!types) {
    hipLaunchKernelGGL((gb_count_kernel<IT, float, int32_t, false>), grid, dim3(256), 0, s, b);
  } else if (dtype == AA_F32) {
    if (types->types_are_int64)
      hipLaunchKernelGGL((gb_count_kernel<IT, float, int64_t, true>), grid, dim3(256), 0, s, b);
    else
      hipLaunchKernelGGL((gb_count_kernel<IT, float, int32_t, true>), grid, dim3(256), 0, s, b);
  } else {
    if (types->types_are_int64)
      hipLaunchKernelGGL((gb_count_kernel<IT, double, int64_t, true>), grid, dim3(256), 0, s, b);
    else
      hipLaunchKernelGGL((gb_count_kernel<IT, double, int32_t, true>), grid, dim3(256), 0, s, b);
  }
}

template <typename IT, typename W>
void launch_build_fill(const BuildDev& b, bool typed, const int32_t* rowptr, const BuildOut& o, dim3 grid, hipStream_t s) {
  if (typed)
    hipLaunchKernelGGL((gb_place_kernel<IT, W, true>), grid, dim3(256), 0, s, b, rowptr, o);
  else
    hipLaunchKernelGGL((gb_place_kernel<IT, W, false>), grid, dim3(256), 0, s, b, rowptr, o);
  hipLaunchKernelGGL(gb_sort_kernel, dim3((unsigned)((b.N + 3) / 4)), dim3(256), 0, s, b, rowptr);
  hipLaunchKernelGGL((gb_gather_kernel<IT, W>), grid, dim3(256), 0, s, b, rowptr, o);
}

}  // namespace

extern "C" size_t aa_graph_build_workspace_bytes(int64_t num_atoms, int64_t num_edges) {
  const size_t N = size_t(std::max<int64_t>(0, num_atoms)), E = size_t(std::max<int64_t>(0, num_edges));
  return 3 * align_up(sizeof(int) * (N + 1)) + align_up(sizeof(int) * build_scan_ints(N, E)) + align_up(kTableBytes) +
         align_up(sizeof(int) * kResInts) + 2 * align_up(sizeof(int) * E) + align_up(sizeof(int) * (E + 1));
}

extern "C" int aa_graph_build_count(const aa_edge_list* in, const aa_nl_types* types, void* workspace, size_t workspace_bytes,
                                    int32_t* out_rowptr, int64_t* out_num_edges, int32_t hints3_host[3], int32_t* input_is_sorted,
                                    aa_stream stream) {
  const char* who = "aa_graph_build_count";
  BuildDev b{};
  std::vector<double> rc2;
  if (types) {  // (before the workspace check, like aa_graph_prune_count)
    double r_max = 0.0;
    if (int rc = check_types(types, in ? in->num_atoms : 0, 0.0, who, rc2, r_max)) return rc;
  }
  if (int rc = plan_build(in, types, workspace, workspace_bytes, who, b)) return rc;
  AA_REQUIRE(out_rowptr && out_num_edges, std::string(who) + ": null output");
  hipStream_t s = static_cast<hipStream_t>(stream);
  AA_CHECK_HIP(hipMemsetAsync(b.a0, 0, sizeof(int) * (size_t(b.N) + 1), s));
  AA_CHECK_HIP(hipMemsetAsync(b.res, 0, sizeof(int) * kResInts, s));
  if (types) AA_CHECK_HIP(hipMemcpyAsync(const_cast<double*>(b.p.rc2), rc2.data(), sizeof(double) * rc2.size(), hipMemcpyHostToDevice, s));
  if (b.E > 0) {
    const dim3 grid((unsigned)((b.E + 255) / 256));
    if (in->index_is_int64)
      launch_build_count<int64_t>(b, types, in->dtype, grid, s);
    else
      launch_build_count<int32_t>(b, types, in->dtype, grid, s);
  }
  launch_scan(b.a0, out_rowptr, b.N, b.scan_tmp, s);
  hipLaunchKernelGGL(gt_hints_kernel, dim3(1), dim3(256), 3 * 256 * sizeof(int), s, b.N, out_rowptr, b.res + kResHints);
  if (types && b.E > 0) launch_scan(b.keepf, b.kpos, b.E, b.scan_tmp, s);
  AA_CHECK_HIP(hipGetLastError());
  int32_t total = 0, res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  AA_CHECK_HIP(hipMemcpyAsync(&total, out_rowptr + b.N, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  AA_CHECK_HIP(hipMemcpyAsync(res, b.res, sizeof(res), hipMemcpyDeviceToHost, s));
  AA_CHECK_HIP(hipStreamSynchronize(s));
  AA_REQUIRE(!res[kResBadCenter], std::string(who) + ": edge_index row 0 (centers) holds an index outside [0, num_atoms) at edge " +
                                      std::to_string(res[kResBadCenter] - 1));
  AA_REQUIRE(!res[kResBadNbr], std::string(who) + ": edge_index row 1 (neighbours) holds an index outside [0, num_atoms) at edge " +
                                   std::to_string(res[kResBadNbr] - 1));
  AA_REQUIRE(!res[kResBadType], std::string(who) + ": atom_types outside [0, num_types)");
  *out_num_edges = total;
  if (hints3_host)
    for (int q = 0; q < 3; ++q) hints3_host[q] = res[kResHints + q];
  if (input_is_sorted) *input_is_sorted = res[kResUnsorted] ? 0 : 1;
  return AA_OK;
}

extern "C" int aa_graph_build_fill(const aa_edge_list* in, const aa_nl_types* types, void* workspace, size_t workspace_bytes,
                                   const int32_t* out_rowptr, int32_t* center, int32_t* nbr, int32_t* perm, void* out_shift_vec,
                                   int32_t* t_rowptr, int32_t* t_perm, aa_stream stream) {
  const char* who = "aa_graph_build_fill";
  BuildDev b{};
  AA_REQUIRE(!types || (types->num_types >= 1 && types->num_types <= kMaxTypes), std::string(who) + ": num_types must lie in [1, 64]");
  if (int rc = plan_build(in, types, workspace, workspace_bytes, who, b)) return rc;
  AA_REQUIRE(out_rowptr, std::string(who) + ": null row pointers");
  AA_REQUIRE((center && nbr) || b.E == 0, std::string(who) + ": null output");
  AA_REQUIRE((t_rowptr == nullptr) == (t_perm == nullptr) || (t_rowptr && b.E == 0), std::string(who) + ": t_rowptr and t_perm go together");
  AA_REQUIRE(!out_shift_vec || in->dtype == AA_F32 || in->dtype == AA_F64, std::string(who) + ": bad dtype");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // (flags, keep flags and their prefix sums are where the count call left them; the histogram array becomes the cursor)
  AA_CHECK_HIP(hipMemsetAsync(b.a0, 0, 3 * align_up(sizeof(int) * (size_t(b.N) + 1)), s));
  if (perm) b.permw = perm;
  BuildOut o{center, nbr, perm, out_shift_vec, t_rowptr ? 1 : 0};
  const dim3 grid((unsigned)((b.E + 255) / 256));
  if (b.E > 0 && b.N > 0) {  // (edges without atoms: all out of range, the count call has refused them)
    const bool w64 = in->dtype == AA_F64;
    if (in->index_is_int64) {
      if (w64)
        launch_build_fill<int64_t, uint64_t>(b, types != nullptr, out_rowptr, o, grid, s);
      else
        launch_build_fill<int64_t, uint32_t>(b, types != nullptr, out_rowptr, o, grid, s);
    } else {
      if (w64)
        launch_build_fill<int32_t, uint64_t>(b, types != nullptr, out_rowptr, o, grid, s);
      else
        launch_build_fill<int32_t, uint32_t>(b, types != nullptr, out_rowptr, o, grid, s);
    }
  }
  if (t_rowptr) {
    launch_scan(b.a1, t_rowptr, b.N, b.scan_tmp, s);
    if (b.E > 0 && b.N > 0) {
      hipLaunchKernelGGL(gb_tplace_kernel, grid, dim3(256), 0, s, b, out_rowptr, nbr, t_rowptr, t_perm);
      hipLaunchKernelGGL(gt_sort_kernel, dim3((unsigned)((b.N + 3) / 4)), dim3(256), 0, s, b.N, t_rowptr, t_perm);
    }
  }
  AA_CHECK_HIP(hipGetLastError());
  return AA_OK;
}

namespace aa {
namespace {
__device__ __forceinline__ unsigned long long fp_mix(unsigned long long x) {  // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// fp[0] += sum_k mix(center_k, nbr_k, k), fp[1] += sum_i mix(type_i, i): integer sums, hence independent of the order the
// workgroups arrive in (bit-reproducible), yet every term depends on its position, so a permutation changes the result
template <typename TT>
__global__ __launch_bounds__(256) void graph_fingerprint_kernel(const int64_t* e0, const int64_t* e1, int64_t E, const TT* types, int64_t N,
                                                                unsigned long long* fp) {
  unsigned long long h0 = 0, h1 = 0;
  const int64_t stride = int64_t(gridDim.x) * 256;
  for (int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x; k < E; k += stride)
    h0 += fp_mix(fp_mix((unsigned long long)e0[k] * 0xD6E8FEB86659FD93ull + (unsigned long long)e1[k]) ^ (unsigned long long)k);
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < N; i += stride)
    h1 += fp_mix(((unsigned long long)(int64_t)types[i] << 40) ^ (unsigned long long)i);
  for (int m = 32; m >= 1; m >>= 1) {
    h0 += __shfl_xor(h0, m);
    h1 += __shfl_xor(h1, m);
  }
  if ((threadIdx.x & 63) == 0) {
    if (h0) atomicAdd(&fp[0], h0);
    if (h1) atomicAdd(&fp[1], h1);
  }
}
}  // namespace
}  // namespace aa

extern "C" int aa_graph_fingerprint(const int64_t* edge_index, int64_t row_stride, int64_t num_edges, const void* atom_types,
                                    int types_are_int64, int64_t num_atoms, uint64_t* fp2, aa_stream stream) {
  AA_REQUIRE(fp2 && num_edges >= 0 && num_atoms >= 0 && (num_edges == 0 || edge_index) && (num_atoms == 0 || atom_types),
             "aa_graph_fingerprint: bad argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  AA_CHECK_HIP(hipMemsetAsync(fp2, 0, 2 * sizeof(uint64_t), s));
  const int64_t work = std::max(num_edges, num_atoms);
  if (work == 0) return AA_OK;
  const unsigned nb = unsigned(std::min<int64_t>((work + 255) / 256, 2048));
  auto* out = reinterpret_cast<unsigned long long*>(fp2);
  if (types_are_int64)
    hipLaunchKernelGGL(aa::graph_fingerprint_kernel<int64_t>, dim3(nb), dim3(256), 0, s, edge_index, edge_index + row_stride, num_edges,
                       static_cast<const int64_t*>(atom_types), num_atoms, out);
  else
    hipLaunchKernelGGL(aa::graph_fingerprint_kernel<int32_t>, dim3(nb), dim3(256), 0, s, edge_index, edge_index + row_stride, num_edges,
                       static_cast<const int32_t*>(atom_types), num_atoms, out);
  AA_CHECK_HIP(hipGetLastError());
  return AA_OK;
}
