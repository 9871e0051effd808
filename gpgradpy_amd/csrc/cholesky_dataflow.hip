// Dataflow (left-looking, tile task graph) Cholesky for gfx950: the whole factorisation as ONE launch.
// Replaces scipy.linalg.cho_factor(Kcov_precon, lower=True) (reference Kernel.py:251; LAPACK dpotrf).
// tile_chol_kernel: 64 x 64 tiles (small matrices), tile128_chol_kernel: 128 x 128 tiles.
// This file is the host side -- task lists, grids, flag buffers, launchers, the gpg_launch_* entry points; the kernels are in the
// headers below, one per kernel family, in the order in which this translation unit defines them.
#include "dataflow_common.h"
#include "dataflow_chol64.h"
#include "dataflow_chol128.h"
#include "dataflow_inverse.h"
#include "dataflow_solve.h"

namespace {

// Ticket order of the factorisation's tasks (Mt tile columns, Rt >= Mt tile rows; B matrices interleaved).  Any order in which a
// task comes after the tasks it reads is valid (progress argument at tile_chol_kernel); two are offered:
//   order 0  tile column by tile column, rows top to bottom, the matrices of a batch interleaved column by column;
//   order 1  the same with the critical path pulled forward: in tile column j the tile (j+1, j) comes first and the NEXT diagonal
//            tile (j+1, j+1) right after it -- it only reads tile row j+1, which (j+1, j) completes -- then the rest of column j.
//            The diagonal tile's potrf / L21 / syrk / potrf chain (~100 us under contention) then runs while column j is still in its
//            MFMA loops, instead of after them with the whole column j+1 waiting for its pieces.
// fuse: the sub-diagonal tiles (j+1, j) of the matrix have no task of their own -- the diagonal task (j+1, j+1) of the 64-tile kernel
// computes and publishes them (tile_chol_task); it only reads earlier tile columns and the pieces of diagonal tile (j, j), all with
// smaller tickets.
template <typename F>
static void for_each_chol_task(int Mt, int Rt, int B, int order, F emit /* (b, i, j) */, bool fuse = false) {
  if (order == 0) {
    for (int j = 0; j < Mt; ++j)
      for (int b = 0; b < B; ++b)
        for (int i = j; i < Rt; ++i)
          if (!(fuse && i == j + 1 && i < Mt)) emit(b, i, j);
    return;
  }
  for (int b = 0; b < B; ++b) emit(b, 0, 0);
  for (int j = 0; j < Mt; ++j) {
    const bool next_diag = j + 1 < Mt;
    if (next_diag)
      for (int b = 0; b < B; ++b) { if (!fuse) emit(b, j + 1, j); emit(b, j + 1, j + 1); }
    for (int b = 0; b < B; ++b)
      for (int i = j + (next_diag ? 2 : 1); i < Rt; ++i) emit(b, i, j);
  }
}

// Ticket order of a launch (gpg_ctx::task_order: 0 column-major, 1 critical path first, -1 = measured choice).  With the round-3
// finalisation (a tile whose diagonal tile is complete on arrival takes the one-piece path) it pays to have the diagonal tiles done
// early: order 1 gains 3.7 % on 64 matrices of 2560 columns, 3 % on 16 of 4608, 2.5 % on the 64-tile batches, 1-3 % on one matrix
// of 9216 columns, and loses 1 % on one matrix of 18048 (tools/tile_probe, GPG_PROBE_ORDER, same box, twice).
static int chol_task_order(const gpg_ctx* c, int B) {
  if (c->task_order >= 0) return c->task_order & 1;
  return (B >= 2 || c->Npad < 16384) ? 1 : 0;
}

// Device copy of a task list, cached under `key` for the lifetime of the context: on a miss build(list, bof) fills the task words and
// -- batched launches -- the matrix index of each of them, and both are uploaded back to back ([list | bof]; TileMap::n counts the task
// words).  nullptr: no memory, nothing to launch (gpg_dev_alloc has marked the context; the API call reports the failure).
template <typename F>
static const TileMap* cached_task_list(gpg_ctx* c, const TaskListKey& key, F build /* (std::vector<int>& list, std::vector<int>& bof) */) {
  auto it = c->tilemaps.find(key);
  if (it != c->tilemaps.end()) return &it->second;
  std::vector<int> list, bof;
  build(list, bof);
  TileMap tm{nullptr, (int)list.size()};
  if (!gpg_dev_alloc(c, &tm.dev, sizeof(int) * (list.size() + bof.size()))) return nullptr;
  (void)hipMemcpy(tm.dev, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice);
  if (!bof.empty()) (void)hipMemcpy(tm.dev + list.size(), bof.data(), sizeof(int) * bof.size(), hipMemcpyHostToDevice);
  return &c->tilemaps.emplace(key, tm).first->second;
}

// Tiles (a, b), a >= b, of the lower triangle of an Mt x Mt tile grid, row by row: the tasks of M = -(Sa Sb^T), longest contraction of
// -(W W^T) (smallest a) first.
static const TileMap* lower_tri_tasks(gpg_ctx* c, int Mt) {
  return cached_task_list(c, TaskListKey{GPG_LIST_LOWER_TRI, 0, 0, 0, Mt, 0}, [&](std::vector<int>& list, std::vector<int>&) {
    for (int a = 0; a < Mt; ++a)
      for (int b = 0; b <= a; ++b) list.push_back(a | (b << 16));
  });
}

// Grid of a persistent launch: as many workgroups as the device holds at once (occupancy x compute units), at most one
// per task.  More would only queue behind the resident ones, fewer would leave slots empty; neither affects
// correctness (ticket order, see tile_chol_kernel).
template <typename K>
static int persistent_grid(gpg_ctx* c, K kernel, long ntask, int block = 256) {
  const void* key = reinterpret_cast<const void*>(kernel);
  auto it = c->occupancy.find(key);
  if (it == c->occupancy.end()) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, 0) != hipSuccess || nb < 1) { (void)hipGetLastError(); nb = 1; }
    it = c->occupancy.emplace(key, nb).first;
  }
  long cap = (long)it->second * (c->num_cus > 0 ? c->num_cus : 256);
  if (c->grid_cap > 0 && c->grid_cap < cap) cap = c->grid_cap;                     // overlapped inverse: leaves slots to the launch it waits for
  if (c->max_workgroups > 0 && c->max_workgroups < cap) cap = c->max_workgroups;   // gpg_set_max_workgroups: tests of the progress argument
  return (int)(ntask < cap ? ntask : cap);
}

// Completion flags of the dataflow launches (grown on demand); false: allocation failed, nothing may be launched.
// The buffer is a multiple of 64 bytes long and cleared in such multiples: the runtime's fill then is ONE kernel instead of an aligned
// body plus a tail.
static inline size_t flags_fill(size_t nflag) { return (nflag + 15) & ~(size_t)15; }
static bool ensure_tile_flags(gpg_ctx* c, size_t nflag) {
  nflag = flags_fill(nflag);
  if (c->tile_flags_cap >= nflag && c->tile_flags) return true;
  if (c->tile_flags) (void)hipFree(c->tile_flags);
  c->tile_flags = nullptr;
  c->tile_flags_cap = 0;
  if (!gpg_dev_alloc(c, &c->tile_flags, sizeof(int) * nflag)) return false;
  c->tile_flags_cap = nflag;
  return true;
}

// The flag words of a launch, cleared on c->stream; nullptr: no memory, nothing may be launched.  Ordinarily c->tile_flags, grown on
// demand.  A launch that may serve the overlapped inverse (gpg_overlap_inverse_begin) takes the buffer waiting in chol_flags_override
// instead -- one-shot; it stays valid after the launch -- and records ev_flags behind the fill: from there on the second stream may poll.
static int* cleared_flags(gpg_ctx* c, size_t nflag, bool may_take_override = false) {
  int* fl = nullptr;
  if (may_take_override) { fl = c->chol_flags_override; c->chol_flags_override = nullptr; }
  const bool keep = fl != nullptr;
  if (!keep) {
    if (!ensure_tile_flags(c, nflag)) return nullptr;
    fl = c->tile_flags;
  }
  (void)hipMemsetAsync(fl, 0, sizeof(int) * flags_fill(nflag), c->stream);
  if (keep) (void)hipEventRecord(c->ev_flags, c->stream);
  return fl;
}

// Task list of pair128_chol_kernel for B >= 2 matrices: per tile column j first the diagonal tiles (paired over the matrices), then each
// matrix's tiles below the diagonal in pairs of consecutive rows, then what was left over (at most one ordinary tile per matrix, paired
// over the matrices) and the right-hand-side tile rows (light tasks: paired with each other).  A tile without a partner is listed
// twice (both teams do it).  Every task waits only for tasks of earlier tile columns and for the diagonal tiles of its own column.
static void build_pair_tasks(int Mt, int Rt, int B, std::vector<int>& list, std::vector<int>& bof, int order) {
  auto emit = [&](int ba, int ia, int bb, int ib, int j) {
    list.push_back(ia | (j << 16)); list.push_back(ib | (j << 16));
    bof.push_back(ba); bof.push_back(bb);
  };
  auto emit_diag = [&](int j) { for (int b = 0; b < B; b += 2) emit(b, j, b + 1 < B ? b + 1 : b, j, j); };
  // order 1 (critical path first, as for_each_chol_task): the first pair below the diagonal of tile column j and then the diagonal
  // tiles of column j + 1 go ahead of the rest of column j
  if (order == 1) emit_diag(0);
  for (int j = 0; j < Mt; ++j) {
    if (order != 1) emit_diag(j);
    std::vector<std::pair<int, int>> left;
    const bool ahead = order == 1 && j + 1 < Mt;
    for (int pass = ahead ? 0 : 1; pass < 2; ++pass) {          // pass 0: only the pair that holds row j + 1; pass 1: the others
      for (int b = 0; b < B; ++b) {
        int i = j + 1;
        for (; i + 1 < Mt; i += 2)
          if (!ahead || (pass == 0) == (i == j + 1)) emit(b, i, b, i + 1, j);
        if (i < Mt && (!ahead || (pass == 0) == (i == j + 1))) left.emplace_back(b, i);
      }
      if (pass == 0) {                                          // (a lone row j + 1 -- the last column pair -- pairs over the matrices right away)
        for (size_t k = 0; k < left.size(); k += 2) {
          const auto& a = left[k];
          const auto& bb = k + 1 < left.size() ? left[k + 1] : left[k];
          emit(a.first, a.second, bb.first, bb.second, j);
        }
        left.clear();
        emit_diag(j + 1);
      }
    }
    for (size_t k = 0; k < left.size(); k += 2) {
      const auto& a = left[k];
      const auto& bb = k + 1 < left.size() ? left[k + 1] : left[k];
      emit(a.first, a.second, bb.first, bb.second, j);
    }
    for (int i = Mt; i < Rt; ++i)                               // right-hand-side tile rows (one per matrix with R = 128)
      for (int b = 0; b < B; b += 2) emit(b, i, b + 1 < B ? b + 1 : b, i, j);
  }
}

static bool pair128_wanted(const gpg_ctx* c, int B) {
  if (c->pair_mode == 1) return true;
  if (c->pair_mode != 2) return false;
  // measured (tools/tile_probe, same box, twice; pair kernel without a barrier in its MFMA loop): ahead of tile128_chol_kernel at every
  // batched size -- 64 x 2560 columns +1.3 %, 16 x 4608 +1.7 %, 8 x 9216 +2.6 %, 8 x 12288 +2.7 %, 2 / 5 / 10 x 18048 +2.2 / +1.3 / +2.3 % --
  // and 1-2 % behind it for ONE matrix per launch (9216 ... 68096 columns)
  return B >= 2 || c->Npad >= c->pair_single_cols;
}

// One dataflow factorisation launch on c->stream.
//  * tile 64: tile_chol_kernel; tile 128: tile128_chol_kernel or -- batched launches for which pair128_wanted says so -- pair128_chol_kernel.
//  * batched: B independent matrices of the context's shape (workspaces A + b a_stride, reciprocal pivots dinv + b d_stride, info[b]) in
//    ONE launch.  The task lists of the matrices are interleaved tile column by tile column, so every matrix's dependency chain advances
//    at the same time and the chip is filled by problems whose single factorisation is latency-bound; the order per matrix is unchanged
//    (progress argument holds).  The kernel gets the matrix of every task (batch_of) and the strides, also for B == 1.
//  * not batched: one matrix, batch_of == nullptr and all strides 0 (the kernels branch on batch_of), task list without matrix indices.
// The two forms stay apart for these kernel arguments only; the flag layout differs by tile size: per matrix the tile flags, the abort
// word (that of matrix 0 serves the whole launch) and per diagonal tile four piece flags (64-tiles) or nine (128-tiles: 4 + 4 pieces and
// the L21 flag), then the eight ticket words of the launch.  The overlapped inverse reads these flags from another stream.
struct CholLaunch {
  int tile, B;
  bool batched;
  double* A; size_t a_stride; double* dinv; int d_stride; int* info;
};
static void launch_chol_dataflow(gpg_ctx* c, const CholLaunch& L) {
  const int B = L.B, Mt = c->Npad / L.tile, Rt = c->ld / L.tile;
  if (Mt <= 0) return;
  // fused diagonal tasks (64-tiles) pay while the launch is chain-bound; from ~4000 columns on their doubled MFMA loops are the longer chain
  // (tools/tile_probe: -8 % at 640 / 1280 columns, -5 % at 2560, +5 % at 5120, +30 % at 9216), and batched launches are throughput-bound:
  // the doubled loop costs +27 % there (64 x 1280 columns)
  const bool fuse = L.tile == 64 && c->fuse_subdiag != 0 && B == 1 && Mt <= c->fuse_subdiag_max_tiles;
  // pair128_chol_kernel (512-thread workgroups, two tiles of a tile column each): a quarter less memory traffic than tile128_chol_kernel
  // (87 against 120 GB per cfg3 matrix) and, since its finalisation lost its spill reloads and its MFMA loop its barrier, 1-3 % faster.
  // One very large matrix per launch (cfg5: 532 tile columns): the rows of a tile column still pair up; only its diagonal tile has no
  // partner and is given to both teams (532 of 142 000 tasks).
  const bool pair = L.tile == 128 && L.batched && pair128_wanted(c, B);
  const int order = chol_task_order(c, B);
  const int kind = !L.batched ? GPG_LIST_CHOL : L.tile == 64 ? GPG_LIST_CHOL_BATCH64 : GPG_LIST_CHOL_BATCH128;
  const TileMap* tm = cached_task_list(c, TaskListKey{kind, order, (fuse || pair) ? 1 : 0, L.batched ? B : 0, Mt, Rt},
                                       [&](std::vector<int>& list, std::vector<int>& bof) {
    if (pair) build_pair_tasks(Mt, Rt, B, list, bof, order);
    else for_each_chol_task(Mt, Rt, B, order, [&](int b, int i, int j) { list.push_back(i | (j << 16)); if (L.batched) bof.push_back(b); }, fuse);
  });
  if (!tm) return;
  const int ntask = pair ? tm->n / 2 : tm->n;              // a pair task is two task words
  const size_t per = (size_t)Mt * Rt + 1 + (L.tile == 64 ? 4 : 9) * (size_t)Mt, nflag = per * B + 8;
  // The batched 128-tile launch never takes the override (nor clears it): what the overlapped inverse follows is one tile per workgroup,
  // which is why launch_tile128_chol keeps a single matrix away from the pair kernel while an override is waiting.
  int* const fl = cleared_flags(c, nflag, !(L.tile == 128 && L.batched));
  if (!fl) return;
  const double m = (double)c->N;                           // algorithmic flops: N^3 / 3 of the real matrix, not of the padded one
  gpg_prof_begin(c, GPG_PROF_GEMM_TRAIL, m > 0 ? B * m * m * m / 3.0 : 0.0);
  int* abort_word = fl + (size_t)Mt * Rt;
  const TileCholArgs args{L.A, c->ld, /* c0: always 0 */ 0, Mt, tm->dev, ntask, fl, abort_word + 1, abort_word, fl + (nflag - 8), L.dinv, L.info, c->N,
                          L.batched ? tm->dev + tm->n : nullptr, L.a_stride, L.d_stride, L.batched ? (int)per : 0, fuse ? 1 : 0};
  if (L.tile == 128) c->last_launch_paired = pair;
  if (L.tile == 64)
    hipLaunchKernelGGL(tile_chol_kernel, dim3(persistent_grid(c, tile_chol_kernel, ntask)), dim3(256), 0, c->stream, args);
  else if (pair)
    hipLaunchKernelGGL(pair128_chol_kernel, dim3(persistent_grid(c, pair128_chol_kernel, ntask, 512)), dim3(512), 0, c->stream, args);
  else
    hipLaunchKernelGGL(tile128_chol_kernel, dim3(persistent_grid(c, tile128_chol_kernel, ntask)), dim3(256), 0, c->stream, args);
  gpg_prof_end(c);
}

// The whole matrix (and the rows below it) with the 64-tile kernel.
static void launch_tile_chol(gpg_ctx* c) {
  launch_chol_dataflow(c, CholLaunch{64, 1, false, c->A, 0, c->dinv, 0, c->info});
}
// The whole matrix with the 128-tile kernels.
static void launch_tile128_chol(gpg_ctx* c) {
  c->last_launch_paired = false;
  const bool as_batch = !c->chol_flags_override && pair128_wanted(c, 1);   // (see the override rule in launch_chol_dataflow)
  launch_chol_dataflow(c, CholLaunch{128, 1, as_batch, c->A, 0, c->dinv, 0, c->info});
}
static void launch_chol_batch(gpg_ctx* c, int tile, int B, double* Abase, size_t a_stride, double* dinv_base, int d_stride, int* info_base) {
  launch_chol_dataflow(c, CholLaunch{tile, B, true, Abase, a_stride, dinv_base, d_stride, info_base});
}

// Minv <- -(L L^T)^-1 (lower triangle, leading dimension Npad) from finished factors, through W = L^-T (Npad x Npad): two
// dataflow launches of N^3/3 flops each per matrix (tile128_trinv_kernel, tile128_wwt_kernel).  B matrices at once
// (factor b at Abase + b a_stride with reciprocal pivots dinv_base + b d_stride, W / Minv of matrix b at + b Npad^2;
// task lists interleaved tile column by tile column like the batched factorisation).  false: not applicable / no memory.
// phase 0: both launches on c->stream; 1: W = L^-T only (flag buffer fbuf, factorisation flags lflags: gpg_overlap_inverse_trinv);
// 2: -(W W^T) only (same fbuf); 3: -(W W^T) only, consuming W by its flags while phase 1 is still running (one matrix).
static bool launch_tile128_inverse_batch(gpg_ctx* c, int B, const double* Abase, size_t a_stride, const double* dinv_base, int d_stride,
                                         double* Wbase, double* Mbase, int* info_base, int phase = 0, int* fbuf = nullptr,
                                         int* lflags = nullptr, int lf_stride = 0) {
  const int Mt = c->Npad / 128, ldw = c->Npad;
  if (Mt < 1 || Mt > 0xffff || B < 1) return false;
  const size_t w_stride = (size_t)ldw * c->Npad;
  // small matrices: W = L^-T with 64 x 64 tiles (half the substitution chain per tile column); -(W W^T) stays on 128-tiles
  const bool small = c->inv_tile64_cols > 0 && c->Npad <= c->inv_tile64_cols;
  const int Mt64 = c->Npad / 64;
  // [tasks W | tasks M | matrix of W task | matrix of M task]
  const TileMap* tm = cached_task_list(c, TaskListKey{GPG_LIST_INVERSE, 0, small ? 1 : 0, B, Mt, 0}, [&](std::vector<int>& list, std::vector<int>& bof) {
    const int Mw = small ? Mt64 : Mt;
    for (int i = 0; i < Mw; ++i)                    // W tiles (j, i): tile column by tile column, longest accumulation first
      for (int b = 0; b < B; ++b)
        for (int j = 0; j <= i; ++j) { list.push_back(j | (i << 16)); bof.push_back(b); }
    for (int a = 0; a < Mt; ++a)                    // M tiles (a, b), a >= b: longest contraction (smallest a) first
      for (int b = 0; b < B; ++b)
        for (int bb = 0; bb <= a; ++bb) { list.push_back(a | (bb << 16)); bof.push_back(b); }
  });
  if (!tm) return false;
  const int n2 = B * (Mt * (Mt + 1) / 2);           // tiles of -(W W^T), always 128 x 128
  const int n1 = tm->n - n2;                        // tiles of W
  const int* tasks1 = tm->dev;
  const int* tasks2 = tm->dev + n1;
  const int* bof1 = tm->dev + tm->n;
  const int* bof2 = bof1 + n1;
  const size_t per = small ? (size_t)Mt64 * Mt64 : (size_t)Mt * Mt;
  const size_t nflag = per * B + 16;                // W tile flags per matrix | 9 ones | abort | ticket (trinv) | ticket (wwt)
  int* fl = fbuf;
  if (!fl) {
    if (!ensure_tile_flags(c, nflag)) return false;
    fl = c->tile_flags;
  }
  int* ones = fl + per * B;
  if (phase != 2 && phase != 3) {
    (void)hipMemsetAsync(fl, 0, sizeof(int) * flags_fill(nflag), c->stream);
    (void)hipMemsetD32Async((hipDeviceptr_t)ones, 1, 9, c->stream);
    for (int b = 0; b < B; ++b) gpg_launch_identity(c, Wbase + (size_t)b * w_stride, ldw);
    // overlapped inverse: from here on W's flags, abort word, tickets and identity are in place -- what -(W W^T) on the main stream,
    // launched while this stream is still busy (phase 3), must not start before
    if (phase == 1 && c->ev_winit) (void)hipEventRecord(c->ev_winit, c->stream);
    if (small)
      hipLaunchKernelGGL(tile64_trinv_kernel, dim3(persistent_grid(c, tile64_trinv_kernel, n1)), dim3(256), 0, c->stream,
                         Trinv64Args{Abase, c->ld, dinv_base, Wbase, ldw, Mt64, tasks1, n1, fl, ones + 9, ones + 10, info_base,
                                     B > 1 ? bof1 : nullptr, a_stride, w_stride, d_stride, (int)per, lflags, lf_stride});
    else
      hipLaunchKernelGGL(tile128_trinv_kernel, dim3(persistent_grid(c, tile128_trinv_kernel, n1)), dim3(256), 0, c->stream,
                         TrinvArgs{Abase, c->ld, dinv_base, Wbase, ldw, Mt, tasks1, n1, fl, ones, ones + 9, ones + 10, info_base,
                                   B > 1 ? bof1 : nullptr, a_stride, w_stride, d_stride, (int)per, B == 1 ? lflags : nullptr, lf_stride /* 64-tile columns of the factorisation, 0: 128-tile */});
    if (phase == 1) return true;
  }
  const bool wflags_live = phase == 3;   // -(W W^T) of ONE matrix while W = L^-T is still running on the other stream (same tiling, flags in fl)
  if (small && B == 1) {   // one small matrix: -(W W^T) on 64-tiles too (task list of its own)
    const TileMap* t64 = lower_tri_tasks(c, Mt64);
    if (!t64) return false;
    hipLaunchKernelGGL(tile64_wwt_kernel, dim3(persistent_grid(c, tile64_wwt_kernel, t64->n)), dim3(256), 0, c->stream,
                       (const double*)Wbase, ldw, Mbase, ldw, Mt64, (const int*)t64->dev, t64->n, ones + 11,
                       wflags_live ? fl : (int*)nullptr, ones + 9, info_base);
    return true;
  }
  hipLaunchKernelGGL(tile128_wwt_kernel, dim3(persistent_grid(c, tile128_wwt_kernel, n2)), dim3(256), 0, c->stream,
                     (const double*)Wbase, ldw, Mbase, ldw, Mt, tasks2, n2, ones + 11, B > 1 ? bof2 : (const int*)nullptr, w_stride,
                     (const double*)nullptr, 0, (wflags_live && !small && B == 1) ? fl : (int*)nullptr, ones + 9, info_base);
  return true;
}

static bool launch_tile128_inverse(gpg_ctx* c, double* W, double* Minv) {
  return launch_tile128_inverse_batch(c, 1, c->A, 0, c->dinv, 0, W, Minv, c->info);
}

// ---- pieces of the Frobenius-norm condition number (gpg_cond_fro; reference GpHparaCon.py:209-236) --------------------
// partial[c] = sum over the rows r >= c (r, c < N) of the lower triangle of M of M[r][c]^2, off-diagonal entries twice
__global__ void __launch_bounds__(256) frob_lower_cols_kernel(const double* __restrict__ M, int ld, int N, double* __restrict__ partial) {
  __shared__ double red[4];
  const int c = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double* col = M + (size_t)c * ld;
  double s = 0.0;
  for (int r = c + threadIdx.x; r < N; r += 256) { const double v = col[r]; s += (r == c ? 1.0 : 2.0) * (v * v); }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) red[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[c] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void __launch_bounds__(256) sum_fixed_order_kernel(const double* __restrict__ v, int n, double* __restrict__ out) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += v[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) red[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}
// upper triangle <- transposed lower triangle (32 x 32 tiles through LDS, coalesced both ways)
__global__ void __launch_bounds__(256) symmetrize_kernel(double* __restrict__ M, int ld, int n) {
  __shared__ double t[32][33];
  const int bi = blockIdx.x, bj = blockIdx.y;            // tile (rows 32 bi.., columns 32 bj..), bi > bj strictly below; diagonal tiles in place
  if (bi < bj) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int r = 32 * bi + tx, c = 32 * bj + k;
    t[k][tx] = (r < n && c < n) ? M[(size_t)r + (size_t)c * ld] : 0.0;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int r = 32 * bj + tx, c = 32 * bi + k;       // element (r, c) of the upper part = element (c, r) of the lower part = t[r - 32 bj][c - 32 bi]
    if (r < n && c < n && r < c) M[(size_t)r + (size_t)c * ld] = t[tx][k];
  }
}

// W (rows x Npad, rows a multiple of 64) <- W L^-T with the dataflow kernel; returns false if it does not apply.
// abort word + ticket cleared and the exchange buffer filled with the sentinel: one launch instead of two fills
__global__ void __launch_bounds__(256) vec_solve_prep_kernel(int* __restrict__ flags, unsigned* __restrict__ x, size_t nwords, unsigned pattern) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < 2) flags[i] = 0;
  if (i < nwords) x[i] = pattern;
}

static bool launch_vec_solve(gpg_ctx* c, double* W, int ldw, int R, bool bwd) {
  const int Mt = c->Npad / 64;
  if (!ensure_tile_flags(c, 64)) return false;
  if (c->vec_x_cols < c->Npad || !c->vec_x) {
    if (c->vec_x) (void)hipFree(c->vec_x);
    c->vec_x_cols = 0;
    if (!gpg_dev_alloc(c, &c->vec_x, sizeof(double) * 4 * (size_t)c->Npad)) return false;
    c->vec_x_cols = c->Npad;
  }
  {
    const size_t nwords = (size_t)2 * R * c->Npad;                                             // abort word, ticket; sentinel words
    hipLaunchKernelGGL(vec_solve_prep_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, c->stream, c->tile_flags,
                       reinterpret_cast<unsigned*>(c->vec_x), nwords, (unsigned)(GPG_VEC_SENTINEL & 0xffffffffull));
  }
#define GPG_VEC_LAUNCH(BWD, RR)                                                                                          \
  hipLaunchKernelGGL((vec_solve_kernel<BWD, RR>), dim3(persistent_grid(c, vec_solve_kernel<BWD, RR>, Mt)), dim3(256), 0,  \
                     c->stream, VecSolveArgs{c->A, c->ld, c->dinv, W, ldw, Mt, R, (unsigned long long*)c->vec_x, c->Npad,  \
                                             c->tile_flags, c->tile_flags + 1, c->info})
  if (bwd) { if (R == 1) GPG_VEC_LAUNCH(1, 1); else GPG_VEC_LAUNCH(1, 4); }
  else     { if (R == 1) GPG_VEC_LAUNCH(0, 1); else GPG_VEC_LAUNCH(0, 4); }
#undef GPG_VEC_LAUNCH
  return true;
}

static bool launch_rows_bwd(gpg_ctx* c, double* Z, int ldz, int rows, int valid) {
  if (rows <= 0 || rows % 64 != 0) return false;
  if (valid >= 1 && valid <= 4 && c->Npad / 64 <= 512) return launch_vec_solve(c, Z, ldz, valid, true);
  const int Mt = c->Npad / 64, nrt = rows / 64;
  if ((long)Mt * nrt > c->rows_max_tasks) return false;
  const size_t nflag = (size_t)Mt * nrt + 2;                    // flags, abort word, ticket
  if (!cleared_flags(c, nflag)) return false;
  hipLaunchKernelGGL(rows_bwd_kernel, dim3(persistent_grid(c, rows_bwd_kernel, (long)Mt * nrt)), dim3(256), 0, c->stream,
                     (const double*)c->A, c->ld, (const double*)c->dinv, Z, ldz, Mt, nrt, valid < 0 ? rows : valid, c->tile_flags,
                     c->tile_flags + (nflag - 2), c->tile_flags + (nflag - 1), c->info);
  return true;
}

static bool launch_rows_fwd(gpg_ctx* c, double* W, int ldw, int rows, int valid) {
  if (rows <= 0 || rows % 64 != 0) return false;
  if (valid >= 1 && valid <= 4 && c->Npad / 64 <= 512) return launch_vec_solve(c, W, ldw, valid, false);
  const int Mt = c->Npad / 64, nrt = rows / 64;
  if ((long)Mt * nrt > c->rows_max_tasks) return false;   // beyond: the blocked sweep (or one launch per group of row tiles)
  const size_t nflag = (size_t)Mt * nrt + 2;                    // flags, abort word, ticket
  if (!cleared_flags(c, nflag)) return false;
  hipLaunchKernelGGL(rows_fwd_kernel, dim3(persistent_grid(c, rows_fwd_kernel, (long)Mt * nrt)), dim3(256), 0, c->stream,
                     (const double*)c->A, c->ld, (const double*)c->dinv, W, ldw, Mt, nrt, valid < 0 ? rows : valid, c->tile_flags,
                     c->tile_flags + (nflag - 2), c->tile_flags + (nflag - 1), c->info);
  return true;
}

}  // namespace

void gpg_launch_tile_chol(gpg_ctx* c) {
  launch_tile_chol(c);
  c->last_factor_kernel = 1; c->last_factor_batch = 1;
}
void gpg_launch_tile128_chol(gpg_ctx* c) {
  launch_tile128_chol(c);
  c->last_factor_kernel = c->last_launch_paired ? 3 : 2; c->last_factor_batch = 1;
}
// ---- value + gradient of ONE small matrix: W = L^-T overlapped with the factorisation ------------------------------------------------
// The two chains (factorisation: one diagonal tile after the other; W = L^-T: one tile column after the other) are each latency-bound on
// a small matrix and most of the chip idles through both.  The inverse's first launch goes to the context's lowest-priority stream
// (gpg_ctx::stream_inv) as soon as the factorisation has been enqueued; its tasks wait for the factorisation's diagonal-tile flags, so
// column tile j of W is under way right after tile column j of L.  Progress: both grids are persistent and draw tickets; a W task waits
// only for factorisation tasks (which never wait for W) and for W tasks with lower tickets.  The W launch becomes runnable as soon as
// the factorisation's flags have been cleared -- possibly BEFORE the factorisation kernel is resident -- so its grid is capped at half
// the co-resident capacity (gpg_ctx::grid_cap): whatever the dispatch order, the factorisation finds free slots, advances, and behind
// it the inverse.  Bounded waits apply as everywhere; a timeout here repeats the call once without the overlap (api.hip).
static size_t chol64_per(const gpg_ctx* c) {
  const size_t Mt = c->Npad / 64, Rt = c->ld / 64;
  return Mt * Rt + 1 + 4 * Mt;
}
// flag words of the factorisation launch that is overlapped: B matrices on 64-tiles, or ONE matrix on 128-tiles (large matrices)
static size_t chol64_nflag(const gpg_ctx* c, int B) {
  if (B == 1 && !gpg_single_uses_tile64(c)) {
    const size_t Mt = c->Npad / 128, Rt = c->ld / 128;
    return flags_fill(Mt * Rt + 1 + 9 * Mt + 8);
  }
  return flags_fill(chol64_per(c) * B + 8);
}
// Does a batch of B matrices go to the 128-tile factorisation kernel?  (gpg_launch_tile_chol_batch below decides with this.)
static bool batch_uses_tile128(const gpg_ctx* c, int B) {
  if (c->factor_mode == GPG_FACTOR_TILE64) return false;
  if (c->factor_mode != GPG_FACTOR_AUTO) return true;       // TILE128 (the blocked mode launches no batches)
  return c->Npad > GPG_AUTO_TILE64_MAX_COLS || (c->Npad >= 2048 && (long)B * (c->Npad / 128) >= 320);
}
bool gpg_overlap_inverse_begin(gpg_ctx* c, int B) {
  const bool small_inv = c->inv_tile64_cols > 0 && c->Npad <= c->inv_tile64_cols;   // W on 64-tiles; above (one matrix only): on 128-tiles
  // the factorisation must be one of the dataflow launches that take the flag override: B matrices on 64-tiles, one on 64- or 128-tiles
  // (the 64-tile W reads 64-tile flags: it needs the 64-tile factorisation; the 128-tile W takes either)
  const bool chol_ok = B > 1 ? !batch_uses_tile128(c, B) : (gpg_single_uses_tile64(c) || (gpg_single_uses_tile128(c) && !small_inv));
  if (!c->overlap_inverse || B < 1 || (!small_inv && B > 1) || !chol_ok || c->prof_mask != 0 || c->stream_inv == c->stream || !c->stream_inv)
    return false;
  const size_t Mt64 = c->Npad / 64;
  const size_t need = chol64_nflag(c, B) + flags_fill(Mt64 * Mt64 * B + 16);           // (the 128-tile W needs a quarter of the second term)
  if (c->keep_flags_cap < need) {
    if (c->keep_flags) (void)hipFree(c->keep_flags);
    c->keep_flags = nullptr; c->keep_flags_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&c->keep_flags), sizeof(int) * need) != hipSuccess) { (void)hipGetLastError(); c->keep_flags = nullptr; return false; }
    c->keep_flags_cap = need;
  }
  if (!c->ev_flags && hipEventCreateWithFlags(&c->ev_flags, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (!c->ev_trinv && hipEventCreateWithFlags(&c->ev_trinv, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (!c->ev_winit && hipEventCreateWithFlags(&c->ev_winit, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
  c->chol_flags_override = c->keep_flags;
  return true;
}
bool gpg_overlap_inverse_trinv(gpg_ctx* c, int B, const double* Abase, size_t a_stride, const double* dinv_base, int d_stride, double* Wbase,
                               int* info_base) {
  hipStream_t main_stream = c->stream;
  (void)hipStreamWaitEvent(c->stream_inv, c->ev_flags, 0);          // the factorisation's flags have been cleared
  c->stream = c->stream_inv;
  c->grid_cap = c->num_cus > 0 ? c->num_cus : 256;                 // one workgroup per compute unit: half of the two-per-CU capacity
  c->overlap_used = true;
  // (last argument: per-matrix stride of the factorisation's flags for the batched 64-tile W; for the 128-tile W of one matrix the number of
  // 64-tile columns of the factorisation, 0 when it ran on 128-tiles itself)
  const bool small_inv = c->inv_tile64_cols > 0 && c->Npad <= c->inv_tile64_cols;
  const int lf = small_inv ? (int)chol64_per(c) : (gpg_single_uses_tile64(c) ? c->Npad / 64 : 0);
  const bool ok = launch_tile128_inverse_batch(c, B, Abase, a_stride, dinv_base, d_stride, Wbase, nullptr, info_base, 1,
                                               c->keep_flags + chol64_nflag(c, B), c->keep_flags, lf);
  (void)hipEventRecord(c->ev_trinv, c->stream_inv);
  c->stream = main_stream;
  c->grid_cap = 0;
  return ok;
}
// The factorisation that W = L^-T overlaps has failed (large matrices: the host reads its info word before going on): raise the abort word
// of the W launch; its tasks look at it first and the launch drains within one task.  One matrix.
void gpg_overlap_inverse_cancel(gpg_ctx* c) {
  const bool small_inv = c->inv_tile64_cols > 0 && c->Npad <= c->inv_tile64_cols;
  const size_t Mt = small_inv ? c->Npad / 64 : c->Npad / 128;
  int* ones = c->keep_flags + chol64_nflag(c, 1) + Mt * Mt;                            // layout of launch_tile128_inverse_batch: ... | 9 ones | abort | tickets
  (void)hipMemsetD32Async((hipDeviceptr_t)(ones + 9), 1, 1, c->stream);
  // wait until it has drained: workgroups that were inside a dependency wait report the abort through the info word like a timed-out
  // wait, and the next call clears that word on the main stream -- nothing of this launch may write it afterwards
  (void)hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(c->stream_inv);
}
bool gpg_overlap_inverse_wwt(gpg_ctx* c, int B, const double* Abase, size_t a_stride, const double* dinv_base, int d_stride, double* Wbase,
                             double* Mbase, int* info_base) {
  if (B == 1 && c->overlap_inverse >= 2) {   // -(W W^T) too follows W tile column by tile column (its flags), on the main stream
    // ... but not before W's flags / abort word / tickets have been cleared and W set to the identity on the other stream: keep_flags is
    // reused across calls, its stale content reads "every tile of W is done"
    (void)hipStreamWaitEvent(c->stream, c->ev_winit, 0);
    return launch_tile128_inverse_batch(c, 1, Abase, a_stride, dinv_base, d_stride, Wbase, Mbase, info_base, 3, c->keep_flags + chol64_nflag(c, 1));
  }
  (void)hipStreamWaitEvent(c->stream, c->ev_trinv, 0);
  return launch_tile128_inverse_batch(c, B, Abase, a_stride, dinv_base, d_stride, Wbase, Mbase, info_base, 2, c->keep_flags + chol64_nflag(c, B));
}
bool gpg_launch_tile128_inverse(gpg_ctx* c, double* W, double* Minv) { return launch_tile128_inverse(c, W, Minv); }
// W = L^-T of the factor in c->A alone (phase 1 of the pair above, on c->stream with the context's own flag buffer)
bool gpg_launch_tile128_trinv(gpg_ctx* c, double* W) {
  const double np = (double)c->Npad;
  gpg_prof_begin(c, GPG_PROF_TRSM, np * np * np / 3.0);
  const bool ok = launch_tile128_inverse_batch(c, 1, c->A, 0, c->dinv, 0, W, nullptr, c->info, 1);
  gpg_prof_end(c);
  return ok;
}
// out_dev[0] = squared Frobenius norm of the symmetric N x N matrix whose lower triangle sits in M (leading dimension ld)
void gpg_launch_frob_lower(gpg_ctx* c, const double* M, int ld, double* partial, double* out_dev) {
  hipLaunchKernelGGL(frob_lower_cols_kernel, dim3(c->N), dim3(256), 0, c->stream, M, ld, c->N, partial);
  hipLaunchKernelGGL(sum_fixed_order_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)partial, c->N, out_dev);
}
void gpg_launch_symmetrize(gpg_ctx* c, double* M, int ld) {
  const int nt = (c->Npad + 31) / 32;
  hipLaunchKernelGGL(symmetrize_kernel, dim3(nt, nt), dim3(256), 0, c->stream, M, ld, c->Npad);
}
// M (lower triangle, leading dimension Npad) = - Sa Sb^T for full Npad x Npad operands (leading dimension Npad)
bool gpg_launch_full_abt(gpg_ctx* c, const double* Sa, const double* Sb, double* M) {
  const int Mt = c->Npad / 128;
  const TileMap* tm = lower_tri_tasks(c, Mt);
  if (!tm) return false;
  if (!ensure_tile_flags(c, 16)) return false;
  (void)hipMemsetAsync(c->tile_flags, 0, sizeof(int) * 16, c->stream);
  hipLaunchKernelGGL(tile128_wwt_kernel, dim3(persistent_grid(c, tile128_wwt_kernel, tm->n)), dim3(256), 0, c->stream, Sa, c->Npad, M,
                     c->Npad, Mt, (const int*)tm->dev, tm->n, c->tile_flags, (const int*)nullptr, (size_t)0, Sb, 1, (int*)nullptr, (int*)nullptr,
                     (int*)nullptr);
  return true;
}
bool gpg_launch_tile128_inverse_batch(gpg_ctx* c, int B, const double* Abase, size_t a_stride, const double* dinv_base, int d_stride,
                                      double* Wbase, double* Mbase, int* info_base) {
  return launch_tile128_inverse_batch(c, B, Abase, a_stride, dinv_base, d_stride, Wbase, Mbase, info_base);
}
bool gpg_launch_rows_fwd(gpg_ctx* c, double* W, int ldw, int rows, int valid) { return launch_rows_fwd(c, W, ldw, rows, valid); }
bool gpg_launch_rows_bwd(gpg_ctx* c, double* Z, int ldz, int rows, int valid) { return launch_rows_bwd(c, Z, ldz, rows, valid); }
void gpg_launch_tile_chol_batch(gpg_ctx* c, int B, double* Abase, size_t a_stride, double* dinv_base, int d_stride,
                                int* info_base) {
  // Which tile size: a forced mode decides; otherwise the 128-tile kernel (higher MFMA rate per workgroup, longer
  // dependency chain per column) as soon as the batch puts enough of its tasks in flight to hide that chain
  // (measured, tools/tile_probe 5 / 6: 2560 columns x 8 matrices 21 TF against 28 for the 64-tile kernel, x 32
  // matrices 37 against 33; 4608 x 8: 42 / 39; 9216 x 8: 59 / 47).
  const bool use128 = batch_uses_tile128(c, B);
  launch_chol_batch(c, use128 ? 128 : 64, B, Abase, a_stride, dinv_base, d_stride, info_base);
  c->last_factor_kernel = use128 ? (c->last_launch_paired ? 3 : 2) : 1;
  c->last_factor_batch = B;
}
