/* TEST HOST, plain C99: the block-wise step ("Frames larger than the workspace") through the plain ABI -- what a LAMMPS pair style whose
 * frame does not fit one workspace does with include/allegro_amd.h.  Same frame file as host_c99.c (the `pair_allegro` ghost-atom
 * layout); the frame is stepped whole (aa_model_energy_forces), as ONE block (must agree bit for bit) and cut greedily into blocks of
 * at most `cap` edges (must agree within 2 x tol x scale, like the reference's outputs within tol x scale).
 *
 *   host_blocked_c99 <model file> <frame file> [tolerance] [cap]
 *
 * Build (tests/test_blocked_host.py): as host_c99.c.                                                                              */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "allegro_amd.h"

#define CHECK_AA(call)                                                                  \
  do {                                                                                  \
    int rc_ = (call);                                                                   \
    if (rc_ != AA_OK) {                                                                 \
      fprintf(stderr, "%s -> %d: %s\n", #call, rc_, aa_last_error());                   \
      return 2;                                                                         \
    }                                                                                   \
  } while (0)
#define CHECK_HIP(call)                                                                 \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      fprintf(stderr, "%s -> %s\n", #call, hipGetErrorString(e_));                      \
      return 2;                                                                         \
    }                                                                                   \
  } while (0)

static void* dev_copy(const void* host, size_t bytes) {
  void* d = NULL;
  if (hipMalloc(&d, bytes ? bytes : 4) != hipSuccess) return NULL;
  if (bytes && hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return NULL;
  return d;
}

/* max |a - b| over n values (1e30 for a NaN), and the scale max(1, max |b|) */
static double max_diff(const float* a, const float* b, int64_t n, double* scale) {
  double d = 0, s = 1;
  for (int64_t i = 0; i < n; ++i) {
    if (isnan(a[i]) || isnan(b[i])) d = 1e30;
    else if (fabs((double)a[i] - b[i]) > d) d = fabs((double)a[i] - b[i]);
    if (fabs(b[i]) > s) s = fabs(b[i]);
  }
  if (scale) *scale = s;
  return d;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s model.aamodel frame.bin [tol] [cap]\n", argv[0]);
    return 2;
  }
  const double tol = argc > 3 ? atof(argv[3]) : 5e-5;

  /* ---- the frame (host_c99.c) ---------------------------------------------------------------------------------- */
  FILE* fp = fopen(argv[2], "rb");
  char magic[8];
  int64_t hdr[3];
  if (!fp || fread(magic, 1, 8, fp) != 8 || memcmp(magic, "AAFRAME1", 8) != 0 || fread(hdr, 8, 3, fp) != 3) {
    fprintf(stderr, "bad frame file\n");
    return 2;
  }
  const int64_t N = hdr[0], E = hdr[1], nlocal = hdr[2];
  float* pos = (float*)malloc(sizeof(float) * 3 * (size_t)N);
  int32_t* center = (int32_t*)malloc(sizeof(int32_t) * (size_t)E);
  int32_t* nbr = (int32_t*)malloc(sizeof(int32_t) * (size_t)E);
  int32_t* types = (int32_t*)malloc(sizeof(int32_t) * (size_t)N);
  float* e_ref = (float*)malloc(sizeof(float) * (size_t)N);
  float* f_ref = (float*)malloc(sizeof(float) * 3 * (size_t)N);
  if (fread(pos, 4, 3 * (size_t)N, fp) != 3 * (size_t)N || fread(center, 4, (size_t)E, fp) != (size_t)E ||
      fread(nbr, 4, (size_t)E, fp) != (size_t)E || fread(types, 4, (size_t)N, fp) != (size_t)N ||
      fread(e_ref, 4, (size_t)N, fp) != (size_t)N || fread(f_ref, 4, 3 * (size_t)N, fp) != 3 * (size_t)N) {
    fprintf(stderr, "truncated frame file\n");
    return 2;
  }
  fclose(fp);
  int32_t* rowptr = (int32_t*)calloc((size_t)N + 1, sizeof(int32_t));
  int32_t* trow = (int32_t*)calloc((size_t)N + 1, sizeof(int32_t));
  int32_t* tperm = (int32_t*)malloc(sizeof(int32_t) * (size_t)(E ? E : 1));
  int64_t max_degree = 0;
  for (int64_t e = 0; e < E; ++e) {
    if (e > 0 && center[e] < center[e - 1]) {
      fprintf(stderr, "edges must be grouped by center atom\n");
      return 2;
    }
    rowptr[center[e] + 1]++;
    trow[nbr[e] + 1]++;
  }
  for (int64_t n = 0; n < N; ++n) {
    if (rowptr[n + 1] > max_degree) max_degree = rowptr[n + 1];
    rowptr[n + 1] += rowptr[n];
    trow[n + 1] += trow[n];
  }
  {
    int32_t* cur = (int32_t*)malloc(sizeof(int32_t) * (size_t)(N + 1));
    memcpy(cur, trow, sizeof(int32_t) * (size_t)(N + 1));
    for (int64_t e = 0; e < E; ++e) tperm[cur[nbr[e]]++] = (int32_t)e;
    free(cur);
  }
  /* ---- the cuts: the host built the list, so it holds the row pointers.  Greedy: a block takes atoms while it stays within `cap`
   *      edges (one atom always fits: cap >= max_degree); the ghost atoms, which have no edges, ride along with the last block */
  const int64_t cap = argc > 4 ? atoll(argv[4]) : 3 * max_degree;
  if (cap < max_degree) {
    fprintf(stderr, "cap %lld is below the largest degree %lld\n", (long long)cap, (long long)max_degree);
    return 2;
  }
  int64_t* block_atoms = (int64_t*)malloc(sizeof(int64_t) * ((size_t)N + 2));
  int64_t* block_edges = (int64_t*)malloc(sizeof(int64_t) * ((size_t)N + 2));
  int32_t B = 0;
  int64_t largest = 0;
  block_atoms[0] = 0;
  block_edges[0] = 0;
  for (int64_t a = 0; a < N;) {
    int64_t a1 = a;
    while (a1 < N && rowptr[a1 + 1] - rowptr[a] <= cap) ++a1;
    ++B;
    block_atoms[B] = a1;
    block_edges[B] = rowptr[a1];
    if (block_edges[B] - block_edges[B - 1] > largest) largest = block_edges[B] - block_edges[B - 1];
    a = a1;
  }

  /* ---- the model ----------------------------------------------------------------------------------------------- */
  aa_model_file* mf = NULL;
  CHECK_AA(aa_model_file_open(argv[1], &mf));
  const aa_model_config* cfg = aa_model_file_config(mf);
  if (cfg->dtype != AA_F32) {
    fprintf(stderr, "this test host handles fp32 models\n");
    return 2;
  }
  aa_model_plan* plan = NULL;
  CHECK_AA(aa_model_plan_create(cfg, &plan));
  hipStream_t stream;
  CHECK_HIP(hipStreamCreate(&stream));
  const size_t wbytes = aa_model_weights_bytes(plan);
  void* blob = NULL;
  CHECK_HIP(hipMalloc(&blob, wbytes));
  CHECK_AA(aa_model_pack_weights(plan, aa_model_file_weights(mf), blob, wbytes, stream));
  /* three workspaces: the whole frame, the frame as one block, the frame in blocks of <= cap edges */
  const size_t ws_bytes = aa_model_workspace_bytes(plan, N, E, 1);
  const size_t ws1_bytes = aa_model_blocked_workspace_bytes(plan, N, E, E, 1);
  const size_t wsb_bytes = aa_model_blocked_workspace_bytes(plan, N, E, largest, 1);
  void *ws = NULL, *ws1 = NULL, *wsb = NULL;
  CHECK_HIP(hipMalloc(&ws, ws_bytes ? ws_bytes : 4));
  CHECK_HIP(hipMalloc(&ws1, ws1_bytes ? ws1_bytes : 4));
  /* (allocated one edge larger: the wrong cut at the end moves one edge from block 0 to block 1) */
  const size_t wsb_wrong_bytes = aa_model_blocked_workspace_bytes(plan, N, E, largest + 1, 1);
  CHECK_HIP(hipMalloc(&wsb, wsb_wrong_bytes ? wsb_wrong_bytes : 4));

  void *d_pos = dev_copy(pos, sizeof(float) * 3 * (size_t)N), *d_center = dev_copy(center, sizeof(int32_t) * (size_t)E),
       *d_nbr = dev_copy(nbr, sizeof(int32_t) * (size_t)E), *d_rowptr = dev_copy(rowptr, sizeof(int32_t) * ((size_t)N + 1)),
       *d_types = dev_copy(types, sizeof(int32_t) * (size_t)N), *d_trow = dev_copy(trow, sizeof(int32_t) * ((size_t)N + 1)),
       *d_tperm = dev_copy(tperm, sizeof(int32_t) * (size_t)E);
  void *d_e = NULL, *d_f = NULL, *d_w9 = NULL, *d_wn = NULL;
  CHECK_HIP(hipMalloc(&d_e, sizeof(float) * (size_t)N));
  CHECK_HIP(hipMalloc(&d_f, sizeof(float) * 3 * (size_t)N));
  CHECK_HIP(hipMalloc(&d_w9, sizeof(float) * 9));
  CHECK_HIP(hipMalloc(&d_wn, sizeof(float) * 9 * (size_t)N));
  if (!d_pos || !d_center || !d_nbr || !d_rowptr || !d_types || !d_trow || !d_tperm) {
    fprintf(stderr, "device allocation failed\n");
    return 2;
  }
  aa_graph g;
  memset(&g, 0, sizeof g);
  g.num_atoms = N;
  g.num_edges = E;
  g.center = (const int32_t*)d_center;
  g.nbr = (const int32_t*)d_nbr;
  g.rowptr = (const int32_t*)d_rowptr;
  g.types = (const int32_t*)d_types;
  g.shift_vec = NULL;
  g.t_rowptr = (const int32_t*)d_trow;
  g.t_perm = (const int32_t*)d_tperm;
  g.atom_begin = 0; /* 0, 0 = all atoms: the whole-frame step then visits the atoms the one-block step visits (the blocked call does not */
  g.atom_end = 0;   /* read the hint; the ghost atoms are centers without edges)                                                       */
  g.max_degree = max_degree;

  const size_t nb_e = sizeof(float) * (size_t)N, nb_f = 3 * nb_e, nb_wn = 9 * nb_e;
  float *e0 = (float*)malloc(nb_e), *f0 = (float*)malloc(nb_f), *wn0 = (float*)malloc(nb_wn), w0[9];
  float *e1 = (float*)malloc(nb_e), *f1 = (float*)malloc(nb_f), *wn1 = (float*)malloc(nb_wn), w1[9];
  float *eb = (float*)malloc(nb_e), *fb = (float*)malloc(nb_f), *wnb = (float*)malloc(nb_wn), wb[9];

  /* ---- the whole frame ----------------------------------------------------------------------------------------- */
  CHECK_AA(aa_model_energy_forces(plan, blob, &g, d_pos, ws, ws_bytes, d_e, d_f, stream));
  CHECK_AA(aa_model_virial(plan, &g, ws, ws_bytes, d_w9, stream));
  CHECK_AA(aa_model_atom_virial(plan, &g, ws, ws_bytes, AA_ATOM_VIRIAL_NEIGHBOR, d_wn, stream));
  CHECK_AA(aa_model_check(plan, stream));
  CHECK_HIP(hipMemcpy(e0, d_e, nb_e, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(f0, d_f, nb_f, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(w0, d_w9, sizeof w0, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(wn0, d_wn, nb_wn, hipMemcpyDeviceToHost));

  /* ---- as ONE block: the same launches on the same numbers ----------------------------------------------------- */
  {
    const int64_t one_atoms[2] = {0, N}, one_edges[2] = {0, E};
    CHECK_AA(aa_model_energy_forces_blocked(plan, blob, &g, d_pos, 1, one_atoms, one_edges, ws1, ws1_bytes, d_e, d_f, stream));
    CHECK_AA(aa_model_blocked_virial(plan, &g, E, ws1, ws1_bytes, d_w9, stream));
    CHECK_AA(aa_model_blocked_atom_virial(plan, &g, E, ws1, ws1_bytes, AA_ATOM_VIRIAL_NEIGHBOR, d_wn, stream));
    CHECK_AA(aa_model_check(plan, stream));
    CHECK_HIP(hipMemcpy(e1, d_e, nb_e, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(f1, d_f, nb_f, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(w1, d_w9, sizeof w1, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(wn1, d_wn, nb_wn, hipMemcpyDeviceToHost));
  }
  int bad = 0;
  if (memcmp(e1, e0, nb_e) != 0 || memcmp(f1, f0, nb_f) != 0 || memcmp(w1, w0, sizeof w0) != 0 || memcmp(wn1, wn0, nb_wn) != 0) {
    printf("host_blocked_c99: ONE block differs from the whole-frame step (max|dE_i| %.3e, max|dF| %.3e)\n", max_diff(e1, e0, N, NULL),
           max_diff(f1, f0, 3 * N, NULL));
    bad = 1;
  } else {
    printf("host_blocked_c99: one block == whole frame, bit for bit (E_i, F, virial, per-atom virial)\n");
  }

  /* ---- in B blocks --------------------------------------------------------------------------------------------- */
  CHECK_AA(aa_model_energy_forces_blocked(plan, blob, &g, d_pos, B, block_atoms, block_edges, wsb, wsb_bytes, d_e, d_f, stream));
  CHECK_AA(aa_model_blocked_virial(plan, &g, largest, wsb, wsb_bytes, d_w9, stream));
  CHECK_AA(aa_model_blocked_atom_virial(plan, &g, largest, wsb, wsb_bytes, AA_ATOM_VIRIAL_NEIGHBOR, d_wn, stream));
  CHECK_AA(aa_model_check(plan, stream)); /* synchronises; every cut verified on the device */
  CHECK_HIP(hipMemcpy(eb, d_e, nb_e, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(fb, d_f, nb_f, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(wb, d_w9, sizeof wb, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(wnb, d_wn, nb_wn, hipMemcpyDeviceToHost));
  double se, sf, sw, swn, sre, srf;
  const double de = max_diff(eb, e0, N, &se), df = max_diff(fb, f0, 3 * N, &sf), dw = max_diff(wb, w0, 9, &sw),
               dwn = max_diff(wnb, wn0, 9 * N, &swn);
  const double dre = max_diff(eb, e_ref, N, &sre), drf = max_diff(fb, f_ref, 3 * N, &srf);
  printf("host_blocked_c99: N=%lld (local %lld) E=%lld max_degree=%lld -> %d blocks of <= %lld edges (largest %lld); workspace %zu bytes "
         "instead of %zu\n", (long long)N, (long long)nlocal, (long long)E, (long long)max_degree, (int)B, (long long)cap, (long long)largest,
         wsb_bytes, ws_bytes);
  printf("host_blocked_c99: blocked vs whole frame: max|dE_i|=%.3e max|dF|=%.3e max|dW|=%.3e max|dW_n|=%.3e  (bound 2 x %.1e x scale)\n", de,
         df, dw, dwn, tol);
  printf("host_blocked_c99: blocked vs reference:   max|dE_i|=%.3e max|dF|=%.3e  (bound %.1e x scale)\n", dre, drf, tol);
  if (!(de <= 2 * tol * se) || !(df <= 2 * tol * sf) || !(dw <= 2 * tol * sw) || !(dwn <= 2 * tol * swn)) bad = 1;
  if (!(dre <= tol * sre) || !(drf <= tol * srf)) bad = 1;
  if (B < 2 || wsb_bytes >= ws_bytes) {
    printf("host_blocked_c99: the cut did not split the frame (B = %d)\n", (int)B);
    bad = 1;
  }

  /* ---- a wrong cut must fail loudly: NaN in the same call, the block named by aa_model_check --------------------- */
  if (B >= 2 && block_edges[1] > 0) {
    block_edges[1] -= 1; /* not the row pointer of block_atoms[1] any more */
    CHECK_AA(aa_model_energy_forces_blocked(plan, blob, &g, d_pos, B, block_atoms, block_edges, wsb, wsb_wrong_bytes, d_e, d_f, stream));
    const int rc = aa_model_check(plan, stream);
    CHECK_HIP(hipMemcpy(eb, d_e, nb_e, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(fb, d_f, nb_f, hipMemcpyDeviceToHost));
    int64_t n_nan = 0;
    for (int64_t n = 0; n < N; ++n) n_nan += isnan(eb[n]) ? 1 : 0;
    for (int64_t i = 0; i < 3 * N; ++i) n_nan += isnan(fb[i]) ? 1 : 0;
    printf("host_blocked_c99: wrong cut -> aa_model_check = %d (%s), %lld of %lld outputs NaN\n", rc, rc ? aa_last_error() : "ok",
           (long long)n_nan, (long long)(4 * N));
    if (rc != AA_ERR_INVALID || n_nan != 4 * N || !strstr(aa_last_error(), "block 0")) bad = 1;
    block_edges[1] += 1;
  }
  aa_model_plan_destroy(plan);
  aa_model_file_close(mf);
  {
    void* dev[] = {blob, ws, ws1, wsb, d_pos, d_center, d_nbr, d_rowptr, d_types, d_trow, d_tperm, d_e, d_f, d_w9, d_wn};
    void* host[] = {pos, center, nbr, types, e_ref, f_ref, rowptr, trow, tperm, block_atoms, block_edges, e0, f0, wn0, e1, f1, wn1, eb, fb, wnb};
    for (size_t i = 0; i < sizeof dev / sizeof dev[0]; ++i) (void)hipFree(dev[i]);
    for (size_t i = 0; i < sizeof host / sizeof host[0]; ++i) free(host[i]);
    (void)hipStreamDestroy(stream);
  }
  printf(bad ? "host_blocked_c99: FAILED\n" : "host_blocked_c99: OK\n");
  return bad;
}
