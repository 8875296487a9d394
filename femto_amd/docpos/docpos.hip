// docpos.hip -- proximity: THEN / WITHIN / OR of (document, offset in document) lists, and the distinct documents of such lists.
// The reference's thenResults / withinResults (src/main/results.c:732 / 842) and unionResults on RESULT_TYPE_DOC_OFFSETS
// (:497).  include/femto_amd.h "positional operators" states the semantics; DESIGN.md "Positional operators" the layout.
//
// CLOSED FORM.  The reference's two-pointer loops compare every left element l with exactly one right element, the first r >= l
// of its document, and every right element r with exactly one left element, the first l > r of its document.  In the stable
// merge of the two lists (a before b on ties) an output taken from a at split (i, j) has b[j] = the first element of b that is
// >= a[i], and an output taken from b has a[i] = the first element of a that is > b[j]: one merge-path search per merged position
// gives the element, its partner and its place in the (ascending) output.  a[i - 1] == b[j] tells an element of b that stands
// in both lists: WITHIN and OR write such a position once, from a.
//
// TILES.  The unit of work is a tile of kTile merged positions of one job; one workgroup of 256 finds the tile's two corner
// splits by diagonal searches in HBM, stages the slices of a and b between them in LDS (with a[i0 - 1], a[i1] and b[j1]: the
// partners at the tile's edges), and every lane searches its kTile / 256 positions there.  How many tiles a call has is known on
// the device only, so nothing is sized by it: the tiles are dealt, in order, into kChunks chunks of equal tile counts (one tile
// each while there are at most kChunks tiles), a persistent grid takes the chunks, and a workgroup walks its chunk's tiles in
// order.  Count pass (per chunk: its outputs; per job: the outputs of its chunk in front of its first tile), a scan over the
// chunks, the jobs' starts, write pass with the running slot: no atomics, a deterministic order.
//
// Both diagonal searches are merge_path_split of ../common/ragged.hpp over pair_le (64-bit indexes in HBM, int in LDS); the
// launches, the host forms' checks and the copy back are ../common/host_common.hpp.  rank_rounds stays here: it ranks kRounds
// flags per thread with one barrier, which is this tile's shape and nobody else's.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../csrc/api_internal.hpp"
#include "../common/host_common.hpp"
#include "../common/block.hpp"

namespace femto_amd {
namespace {

constexpr int kTile = 2048;                  // merged positions per tile: (kTile + 4) staged pairs = 32.1 KB of LDS, four workgroups per CU
constexpr int kRounds = kTile / 256;
constexpr int kStage = kTile + 4;
constexpr int64_t kChunks = 32768;

struct TArgs {
  int64_t njobs;
  // positional jobs
  const int64_t *a_doc, *a_off, *a_start;
  const int32_t* a_n;
  const int64_t *b_doc, *b_off, *b_start;
  const int32_t* b_n;
  const int32_t *op, *distance;
  // lists whose documents are wanted
  const int64_t* l_starts;     // njobs + 1
  const int64_t* l_doc;
  // the tile machinery
  int64_t* tile_counts;        // njobs
  const int64_t* tile_starts;  // njobs + 1
  int64_t* chunk_counts;       // kChunks
  const int64_t* chunk_starts; // kChunks + 1
  int64_t* job_local;          // njobs
  // results
  int64_t* res_starts;         // njobs + 1
  int64_t *res_doc, *res_off;  // res_off NULL: documents
  int64_t res_capacity;
  int64_t* res_total;
};

enum { kPositional = 0, kDocuments = 1 };

template <int kKind>
__device__ __forceinline__ int64_t job_size(const TArgs& A, int64_t k) {
  if (kKind == kPositional) {
    const int64_t na = A.a_n[k] > 0 ? A.a_n[k] : 0, nb = A.b_n[k] > 0 ? A.b_n[k] : 0;
    return na + nb;
  }
  const int64_t s = A.l_starts[k], e = A.l_starts[k + 1];
  return s >= 0 && e > s ? e - s : 0;
}

template <int kKind>
__global__ __launch_bounds__(256) void docpos_tilecount_kernel(const TArgs A) {
  const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (k < A.njobs) A.tile_counts[k] = (job_size<kKind>(A, k) + kTile - 1) / kTile;
}

__device__ __forceinline__ bool pair_le(int64_t ad, int64_t ao, int64_t bd, int64_t bo) { return ad < bd || (ad == bd && ao <= bo); }

struct Lds {
  int64_t doc[kStage], off[kStage];
  int64_t split[2];
  int cnt[kRounds * 4];
};

// slots of the kept elements of a tile, in the order round, thread: returns the tile's count; slot[r] is exclusive within the tile
__device__ __forceinline__ int rank_rounds(const bool (&keep)[kRounds], Lds& S, int (&slot)[kRounds]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long m[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; r++) {
    m[r] = __ballot(keep[r]);
    if (lane == 0) S.cnt[r * 4 + w] = __popcll(m[r]);
  }
  __syncthreads();
  int acc = 0;
#pragma unroll
  for (int r = 0; r < kRounds; r++) {
#pragma unroll
    for (int ww = 0; ww < 4; ww++) {
      if (ww == w) slot[r] = acc + __popcll(m[r] & ((1ull << lane) - 1ull));
      acc += S.cnt[r * 4 + ww];
    }
  }
  return acc;
}

// merged positions [p0, p0 + kTile) of job k; the results go to out0 + their rank
template <bool kWrite>
__device__ __forceinline__ int positional_tile(const TArgs& A, int64_t k, int64_t p0, int64_t out0, Lds& S) {
  const int64_t na = A.a_n[k] > 0 ? A.a_n[k] : 0, nb = A.b_n[k] > 0 ? A.b_n[k] : 0;
  const int64_t* __restrict__ ad = A.a_doc + A.a_start[k];
  const int64_t* __restrict__ ao = A.a_off + A.a_start[k];
  const int64_t* __restrict__ bd = A.b_doc + A.b_start[k];
  const int64_t* __restrict__ bo = A.b_off + A.b_start[k];
  const int op = A.op[k];
  const int64_t d = A.distance[k], dist = d < 0 ? -d : d;
  const int64_t p1 = p0 + kTile < na + nb ? p0 + kTile : na + nb;
  if (threadIdx.x < 2) {
    // the corner's split (p = 0 and p = na + nb search nothing: a job of one tile reads nothing in HBM here)
    S.split[threadIdx.x] = merge_path_split(threadIdx.x ? p1 : p0, na, nb, [&](int64_t i, int64_t j) { return pair_le(ad[i], ao[i], bd[j], bo[j]); });
  }
  __syncthreads();
  const int64_t i0 = S.split[0], i1 = S.split[1], j0 = p0 - i0, j1 = p1 - i1;
  // staged: a[ia0, ia1) then b[j0, jb1): the slices between the splits, a[i0 - 1], a[i1] and b[j1] (at most kTile + 3 pairs)
  const int64_t ia0 = i0 > 0 ? i0 - 1 : 0, ia1 = i1 < na ? i1 + 1 : na, jb1 = j1 < nb ? j1 + 1 : nb;
  const int la_all = int(ia1 - ia0), lb_all = int(jb1 - j0);
  for (int t = threadIdx.x; t < la_all + lb_all; t += 256) {
    const bool is_a = t < la_all;
    const int64_t x = is_a ? ia0 + t : j0 + (t - la_all);
    S.doc[t] = is_a ? ad[x] : bd[x];
    S.off[t] = is_a ? ao[x] : bo[x];
  }
  __syncthreads();
  const int abase = int(i0 - ia0), bbase = la_all;       // a[i0 + x] = S[abase + x], b[j0 + y] = S[bbase + y]
  const int la = int(i1 - i0), lb = int(j1 - j0);
  bool keep[kRounds];
  int64_t vd[kRounds], vo[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; r++) {
    const int q = r * 256 + int(threadIdx.x);
    keep[r] = false;
    vd[r] = vo[r] = 0;
    if (q < la + lb) {
      const int x = merge_path_split(q, la, lb, [&](int i, int j) { return pair_le(S.doc[abase + i], S.off[abase + i], S.doc[bbase + j], S.off[bbase + j]); });
      const int y = q - x;
      const bool has_a = i0 + x < na, has_b = j0 + y < nb;
      const int64_t a_d = has_a ? S.doc[abase + x] : 0, a_o = has_a ? S.off[abase + x] : 0;
      const int64_t b_d = has_b ? S.doc[bbase + y] : 0, b_o = has_b ? S.off[bbase + y] : 0;
      const bool from_a = has_a && (!has_b || pair_le(a_d, a_o, b_d, b_o));
      if (from_a) {
        // b[j]: the first element of b that is >= a[i]
        const bool near = has_b && b_d == a_d;
        const int64_t width = b_o - a_o;
        vd[r] = a_d;
        vo[r] = a_o;
        keep[r] = op == FEMTO_AMD_DOCPOS_THEN     ? d > 0 && near && width > 0 && width <= dist
                  : op == FEMTO_AMD_DOCPOS_WITHIN ? near && width <= dist
                                                  : op == FEMTO_AMD_DOCPOS_OR;
      } else {
        // a[i]: the first element of a that is > b[j]; a[i - 1] == b[j]: the position stands in both lists
        const bool both = i0 + x > 0 && S.doc[abase + x - 1] == b_d && S.off[abase + x - 1] == b_o;
        const bool near = has_a && a_d == b_d && a_o - b_o <= dist;
        vd[r] = b_d;
        vo[r] = b_o;
        keep[r] = op == FEMTO_AMD_DOCPOS_THEN     ? d < 0 && near
                  : op == FEMTO_AMD_DOCPOS_WITHIN ? near && !both
                                                  : op == FEMTO_AMD_DOCPOS_OR && !both;
      }
    }
  }
  int slot[kRounds];
  const int count = rank_rounds(keep, S, slot);
  if (kWrite) {
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
      const int64_t s = out0 + slot[r];
      if (keep[r] && s >= 0 && s < A.res_capacity) {
        A.res_doc[s] = vd[r];
        A.res_off[s] = vo[r];
      }
    }
  }
  return count;
}

// elements [p0, p0 + kTile) of list k: an element that differs from the one before it (or has none) starts a document
template <bool kWrite>
__device__ __forceinline__ int documents_tile(const TArgs& A, int64_t k, int64_t p0, int64_t out0, Lds& S) {
  const int64_t n = job_size<kDocuments>(A, k);
  const int64_t* __restrict__ doc = A.l_doc + A.l_starts[k];
  bool keep[kRounds];
  int64_t v[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; r++) {
    const int64_t p = p0 + r * 256 + threadIdx.x;
    keep[r] = false;
    v[r] = 0;
    if (p < n) {
      v[r] = doc[p];
      keep[r] = p == 0 || doc[p - 1] != v[r];
    }
  }
  int slot[kRounds];
  const int count = rank_rounds(keep, S, slot);
  if (kWrite) {
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
      const int64_t s = out0 + slot[r];
      if (keep[r] && s >= 0 && s < A.res_capacity) A.res_doc[s] = v[r];
    }
  }
  return count;
}

// persistent grid over the chunks.  kWrite = false: chunk_counts and job_local; true: the results
template <int kKind, bool kWrite>
__global__ __launch_bounds__(256) void docpos_tiles_kernel(const TArgs A) {
  __shared__ Lds S;
  const int64_t* __restrict__ ts = A.tile_starts;
  const int64_t ntiles = ts[A.njobs];
  const int64_t per = ntiles > kChunks ? (ntiles + kChunks - 1) / kChunks : 1;     // tiles per chunk
  for (int64_t c = blockIdx.x; c < kChunks; c += gridDim.x) {
    const int64_t t0 = c * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    int64_t run = kWrite ? A.chunk_starts[c] : 0;
    int64_t k = -1, kbeg = 0, kend = -1;
    for (int64_t t = t0; t < t1; t++) {
      if (t >= kend) {      // the job tile t belongs to: the next one, or the last whose tiles start at or before t
        k = (k >= 0 && k + 1 < A.njobs && ts[k + 2] > t) ? k + 1 : last_start_le(ts, A.njobs, t);
        kbeg = ts[k];
        kend = ts[k + 1];
      }
      if (!kWrite && t == kbeg && threadIdx.x == 0) A.job_local[k] = run;
      __syncthreads();      // (the tile before has read its counts)
      run += kKind == kPositional ? positional_tile<kWrite>(A, k, (t - kbeg) * kTile, run, S) : documents_tile<kWrite>(A, k, (t - kbeg) * kTile, run, S);
    }
    if (!kWrite && threadIdx.x == 0) A.chunk_counts[c] = run;
  }
}

// res_starts[k] = the slot of job k's first tile (of the next job's that has one; the total behind the last), and res_total
__global__ __launch_bounds__(256) void docpos_starts_kernel(const TArgs A) {
  const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (k > A.njobs) return;
  const int64_t ntiles = A.tile_starts[A.njobs], total = A.chunk_starts[kChunks];
  const int64_t per = ntiles > kChunks ? (ntiles + kChunks - 1) / kChunks : 1;
  const int64_t t = A.tile_starts[k];
  A.res_starts[k] = t >= ntiles ? total : A.chunk_starts[t / per] + A.job_local[last_start_le(A.tile_starts, A.njobs, t)];
  if (k == A.njobs) write_total(A.res_total, total, A.res_capacity);
}

// ---- host side --------------------------------------------------------------------------------------------------------------

constexpr const char* kSubject = "positional operators are";

// the passes over the tiles of A's jobs (everything of A but the tile machinery is set)
template <int kKind>
int run_tiles(femto_amd_index* ix, Scratch& S, TArgs A, hipStream_t st) {
  int rc;
  const int64_t n = A.njobs;
  if ((rc = S.noccs64.reserve(size_t(n) * 8)) || (rc = S.out_starts.reserve(size_t(n + 1) * 8)) || (rc = S.keys.reserve(size_t(n) * 8)) ||
      (rc = S.keys2.reserve(size_t(2 * kChunks + 1) * 8)))
    return rc;
  A.tile_counts = S.noccs64.as<int64_t>();
  A.tile_starts = S.out_starts.as<int64_t>();
  A.job_local = S.keys.as<int64_t>();
  A.chunk_counts = S.keys2.as<int64_t>();
  A.chunk_starts = A.chunk_counts + kChunks;
  const int64_t cap = int64_t(ix->num_cus) * 4;      // four workgroups per CU are resident (their LDS)
  const dim3 per_job = blocks_for(n), grid{uint32_t(cap < kChunks ? cap : kChunks)};
  if ((rc = launch(docpos_tilecount_kernel<kKind>, per_job, st, A)) ||
      (rc = device_scan(S.scan, n, A.tile_counts, S.out_starts.as<int64_t>(), 0, st)) ||
      (rc = launch(docpos_tiles_kernel<kKind, false>, grid, st, A)) ||
      (rc = device_scan(S.scan, kChunks, A.chunk_counts, A.chunk_counts + kChunks, 0, st)) || (rc = launch(docpos_starts_kernel, per_job, st, A)))
    return rc;
  return launch(docpos_tiles_kernel<kKind, true>, grid, st, A);
}

int run_docpos(femto_amd_index* ix, Scratch& S, int64_t npairs, const int64_t* d_a_doc, const int64_t* d_a_off, const int64_t* d_a_start,
               const int32_t* d_a_n, const int64_t* d_b_doc, const int64_t* d_b_off, const int64_t* d_b_start, const int32_t* d_b_n,
               const int32_t* d_op, const int32_t* d_distance, int64_t* d_res_starts, int64_t* d_res_doc, int64_t* d_res_off,
               int64_t res_capacity, int64_t* d_res_total, hipStream_t st) {
  TArgs A{};
  A.njobs = npairs;
  A.a_doc = d_a_doc;
  A.a_off = d_a_off;
  A.a_start = d_a_start;
  A.a_n = d_a_n;
  A.b_doc = d_b_doc;
  A.b_off = d_b_off;
  A.b_start = d_b_start;
  A.b_n = d_b_n;
  A.op = d_op;
  A.distance = d_distance;
  A.res_starts = d_res_starts;
  A.res_doc = d_res_doc;
  A.res_off = d_res_off;
  A.res_capacity = res_capacity;
  A.res_total = d_res_total;
  return run_tiles<kPositional>(ix, S, A, st);
}

bool known_op(int32_t op) { return op == FEMTO_AMD_DOCPOS_THEN || op == FEMTO_AMD_DOCPOS_WITHIN || op == FEMTO_AMD_DOCPOS_OR; }

}  // namespace
}  // namespace femto_amd

int femto_amd_docpos_info(int* tile) {
  if (tile) *tile = kTile;
  return FEMTO_AMD_OK;
}

int femto_amd_docpos_chunks(void) { return int(kChunks); }

int femto_amd_docpos_device(femto_amd_index_t* ix, int64_t npairs, const int64_t* d_a_doc, const int64_t* d_a_off, const int64_t* d_a_start,
                            const int32_t* d_a_n, const int64_t* d_b_doc, const int64_t* d_b_off, const int64_t* d_b_start,
                            const int32_t* d_b_n, const int32_t* d_op, const int32_t* d_distance, int64_t* d_res_starts, int64_t* d_res_doc,
                            int64_t* d_res_off, int64_t res_capacity, int64_t* d_res_total, void* stream) {
  API_BEGIN
  if (!ix || npairs < 0 || res_capacity < 0 || !d_res_starts || !d_res_total || (res_capacity && (!d_res_doc || !d_res_off)) ||
      (npairs && (!d_a_doc || !d_a_off || !d_a_start || !d_a_n || !d_b_doc || !d_b_off || !d_b_start || !d_b_n || !d_op || !d_distance)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  if (npairs >= (int64_t(1) << 40)) return set_err(FEMTO_AMD_ERR_PARAM, "too many jobs in one call: split the batch");
  if (!ix->children.empty()) return refuse_multi_device();
  int rc = check_plain_handle(ix, kSubject);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (npairs == 0) return empty_result_async(d_res_starts, d_res_total, st);
  Lease L(ix, st);
  if (!L.s) return L.rc;
  return run_docpos(ix, *L.s, npairs, d_a_doc, d_a_off, d_a_start, d_a_n, d_b_doc, d_b_off, d_b_start, d_b_n, d_op, d_distance, d_res_starts,
                    d_res_doc, d_res_off, res_capacity, d_res_total, st);
  API_END
}

int femto_amd_docpos_documents_device(femto_amd_index_t* ix, int64_t nlists, const int64_t* d_starts, const int64_t* d_pair_doc,
                                      int64_t* d_doc_starts, int64_t* d_docs, int64_t doc_capacity, int64_t* d_total, void* stream) {
  API_BEGIN
  if (!ix || nlists < 0 || doc_capacity < 0 || !d_doc_starts || !d_total || (doc_capacity && !d_docs) || (nlists && (!d_starts || !d_pair_doc)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  if (nlists >= (int64_t(1) << 40)) return set_err(FEMTO_AMD_ERR_PARAM, "too many lists in one call: split the batch");
  if (!ix->children.empty()) return refuse_multi_device();
  int rc = check_plain_handle(ix, kSubject);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (nlists == 0) return empty_result_async(d_doc_starts, d_total, st);
  Lease L(ix, st);
  if (!L.s) return L.rc;
  TArgs A{};
  A.njobs = nlists;
  A.l_starts = d_starts;
  A.l_doc = d_pair_doc;
  A.res_starts = d_doc_starts;
  A.res_doc = d_docs;
  A.res_capacity = doc_capacity;
  A.res_total = d_total;
  return run_tiles<kDocuments>(ix, *L.s, A, st);
  API_END
}

int femto_amd_docpos(femto_amd_index_t* ix0, int64_t npairs, const int64_t* a_doc, const int64_t* a_off, const int64_t* a_start,
                     const int32_t* a_n, const int64_t* b_doc, const int64_t* b_off, const int64_t* b_start, const int32_t* b_n,
                     const int32_t* op, const int32_t* distance, int64_t* res_starts, int64_t** res_doc, int64_t** res_off, int64_t* total) {
  API_BEGIN
  if (!ix0 || npairs < 0 || !res_starts || !res_doc || !res_off || !total ||
      (npairs && (!a_doc || !a_off || !a_start || !a_n || !b_doc || !b_off || !b_start || !b_n || !op || !distance)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  *res_doc = *res_off = nullptr;
  *total = 0;
  res_starts[0] = 0;
  int64_t la, lb, bound = 0;
  int rc = check_list_pairs(npairs, a_start, a_n, b_start, b_n, &la, &lb);
  if (rc) return rc;
  for (int64_t k = 0; k < npairs; k++) {
    if (!known_op(op[k])) return set_err(FEMTO_AMD_ERR_PARAM, "unknown positional operator");
    bound += int64_t(a_n[k]) + b_n[k];
  }
  femto_amd_index* ix = replica0(ix0);
  if ((rc = check_plain_handle(ix, kSubject))) return rc;
  if (npairs == 0) return FEMTO_AMD_OK;
  HIP_TRY(hipSetDevice(ix->device));
  Temp T;
  int64_t *d_ad, *d_ao, *d_bd, *d_bo, *d_as, *d_bs, *d_rs, *d_rd, *d_ro, *d_rt;
  int32_t *d_an, *d_bn, *d_op, *d_di;
  const size_t np = size_t(npairs);
  if ((rc = T.put(&d_ad, a_doc, size_t(la))) || (rc = T.put(&d_ao, a_off, size_t(la))) || (rc = T.put(&d_bd, b_doc, size_t(lb))) ||
      (rc = T.put(&d_bo, b_off, size_t(lb))) || (rc = T.put(&d_as, a_start, np)) || (rc = T.put(&d_bs, b_start, np)) ||
      (rc = T.put(&d_an, a_n, np)) || (rc = T.put(&d_bn, b_n, np)) || (rc = T.put(&d_op, op, np)) || (rc = T.put(&d_di, distance, np)) ||
      (rc = T.get(&d_rs, np + 1)) || (rc = T.get(&d_rd, size_t(bound))) || (rc = T.get(&d_ro, size_t(bound))) || (rc = T.get(&d_rt, 2)))
    return rc;
  Lease L(ix);
  if (!L.s) return L.rc;
  hipStream_t st = L.s->stream;
  if ((rc = run_docpos(ix, *L.s, npairs, d_ad, d_ao, d_as, d_an, d_bd, d_bo, d_bs, d_bn, d_op, d_di, d_rs, d_rd, d_ro, bound, d_rt, st))) return rc;
  return copy_pairs_back(npairs, d_rs, d_rd, d_ro, st, res_starts, res_doc, res_off, total);
  API_END
}

int femto_amd_proximity(femto_amd_index_t* ix0, int64_t npairs, const int32_t* l_plen, const uint16_t* l_pats, const int64_t* l_starts,
                        const int32_t* r_plen, const uint16_t* r_pats, const int64_t* r_starts, const int32_t* op, const int32_t* distance,
                        int max_occs_each, int64_t* res_starts, int64_t** res_doc, int64_t** res_off, int64_t* total) {
  API_BEGIN
  if (!ix0 || npairs < 0 || !res_starts || !res_doc || !res_off || !total ||
      (npairs && (!l_plen || !l_pats || !l_starts || !r_plen || !r_pats || !r_starts || !op || !distance)))
    return set_err(FEMTO_AMD_ERR_PARAM, "bad arguments");
  *res_doc = *res_off = nullptr;
  *total = 0;
  res_starts[0] = 0;
  if (npairs >= (int64_t(1) << 30)) return set_err(FEMTO_AMD_ERR_PARAM, "too many pattern pairs in one call: split the batch");
  int64_t lsyms, rsyms;
  int rc;
  if ((rc = check_patterns(npairs, l_plen, l_pats, l_starts, &lsyms)) || (rc = check_patterns(npairs, r_plen, r_pats, r_starts, &rsyms))) return rc;
  for (int64_t k = 0; k < npairs; k++)
    if (!known_op(op[k])) return set_err(FEMTO_AMD_ERR_PARAM, "unknown positional operator");
  femto_amd_index* ix = replica0(ix0);
  if ((rc = check_plain_handle(ix, kSubject))) return rc;
  if (npairs == 0) return FEMTO_AMD_OK;
  // one batch of 2 * npairs patterns: the left sides, then the right sides (their symbols behind the left sides')
  const int64_t np = 2 * npairs, nsyms = lsyms + rsyms;
  std::vector<int32_t> plen(static_cast<size_t>(np));
  std::vector<int64_t> starts(static_cast<size_t>(np));
  for (int64_t k = 0; k < npairs; k++) {
    plen[size_t(k)] = l_plen[k];
    starts[size_t(k)] = l_starts[k];
    plen[size_t(npairs + k)] = r_plen[k];
    starts[size_t(npairs + k)] = lsyms + r_starts[k];
  }
  HIP_TRY(hipSetDevice(ix->device));
  Temp T;
  int32_t *d_plen, *d_op, *d_di;
  uint16_t* d_pats;
  int64_t *d_starts, *d_pd, *d_po, *d_rs, *d_rd, *d_ro, *d_rt;
  LocatedRows R;      // every result holds at most R.rows pairs
  if ((rc = upload_patterns(T, np, plen.data(), starts.data(), nsyms, {{l_pats, lsyms, 0}, {r_pats, rsyms, lsyms}}, &d_plen, &d_pats, &d_starts)) ||
      (rc = T.put(&d_op, op, size_t(npairs))) || (rc = T.put(&d_di, distance, size_t(npairs))) || (rc = T.get(&d_rs, size_t(npairs) + 1)) ||
      (rc = T.get(&d_rt, 2)) || (rc = locate_rows(ix, T, np, d_plen, d_pats, d_starts, max_occs_each, &R)) ||
      (rc = T.get(&d_pd, size_t(R.rows))) || (rc = T.get(&d_po, size_t(R.rows))) || (rc = T.get(&d_rd, size_t(R.rows))) ||
      (rc = T.get(&d_ro, size_t(R.rows))))
    return rc;
  // the listing (pairs form) takes a scratch of its own and gives it back when it returns: it is enqueued BEFORE this call leases
  // one, so that no thread ever holds a scratch while it waits for another (the pool is bounded: more callers than scratches,
  // each holding one and waiting for a second, would never return)
  if ((rc = femto_amd_doclist_device(ix, np, R.ostarts, R.offs, R.rows, R.tot, nullptr, nullptr, nullptr, nullptr, d_pd, d_po, nullptr, nullptr, nullptr)))
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  Lease L(ix);
  if (!L.s) return L.rc;
  hipStream_t st = L.s->stream;
  // combine: job k = segment k with segment npairs + k of the rows' own layout
  if ((rc = run_docpos(ix, *L.s, npairs, d_pd, d_po, R.ostarts, R.noccs, d_pd, d_po, R.ostarts + npairs, R.noccs + npairs, d_op, d_di, d_rs, d_rd,
                       d_ro, R.rows, d_rt, st)))
    return rc;
  return copy_pairs_back(npairs, d_rs, d_rd, d_ro, st, res_starts, res_doc, res_off, total);
  API_END
}
