// Pure-host planning unit (operator_plans.h): format choice, lattice completion, strip-walk plans, column-blocked mirror, the
// batched path's row order and LDS tiles.  Ordinary C++ on plain data; engine_plans.hip uploads what comes back.
#include "operator_plans.h"

#include <array>
#include <atomic>
#include <numeric>

namespace {

// ---- the index idioms the planners share ---------------------------------------------------------------------------------
inline int64_t row_len(const UnionPattern& A, int64_t r) { return A.ur[r + 1] - A.ur[r]; }

// column distances col - r of row r, ascending; `folded`: into (-n/2, n/2] (a periodic lattice's wrap-around entries)
std::vector<int64_t> row_distances(const UnionPattern& A, int64_t r, bool folded = false) {
  const int64_t n = A.nrows;
  std::vector<int64_t> D((size_t)row_len(A, r));
  for (size_t k = 0; k < D.size(); ++k) {
    int64_t d = (int64_t)A.uc[A.ur[r] + (int64_t)k] - r;
    if (folded && d > n / 2) d -= n;
    if (folded && d <= -(n + 1) / 2) d += n;
    D[k] = d;
  }
  return D;
}

// entries of row r left of the diagonal (the rows are sorted: a prefix)
inline int64_t lower_count(const UnionPattern& A, int64_t r) {
  int64_t nl = 0;
  while (A.ur[r] + nl < A.ur[r + 1] && A.uc[A.ur[r] + nl] < r) ++nl;
  return nl;
}

// does row r carry the same column distances as row `ref`?  `lower_only`: among the entries left of the diagonal
bool same_distances(const UnionPattern& A, int64_t r, int64_t ref, bool lower_only = false) {
  const int64_t len = lower_only ? lower_count(A, ref) : row_len(A, ref);
  if ((lower_only ? lower_count(A, r) : row_len(A, r)) != len) return false;
  const int32_t* a = A.uc.data() + A.ur[r];
  const int32_t* c = A.uc.data() + A.ur[ref];
  const int64_t shift = r - ref;
  for (int64_t k = 0; k < len; ++k)
    if ((int64_t)a[k] - (int64_t)c[k] != shift) return false;
  return true;
}

// sums[i] over rows [0, n): fn(a, b, mine) adds its chunk's counts to `mine`, on the host threads
template <size_t N, class F>
std::array<int64_t, N> parallel_sums(int64_t n, F&& fn, int64_t serial_below = (int64_t)1 << 16) {
  std::array<std::atomic<int64_t>, N> total;
  for (auto& t : total) t.store(0);
  parallel_rows(n, [&](int64_t a, int64_t b) {
    std::array<int64_t, N> mine{};
    fn(a, b, mine);
    for (size_t i = 0; i < N; ++i) total[i].fetch_add(mine[i], std::memory_order_relaxed);
  }, serial_below);
  std::array<int64_t, N> out;
  for (size_t i = 0; i < N; ++i) out[i] = total[i].load();
  return out;
}

// values a row-block layout stores when row r contributes width(r) entries: per 64-row block the widest row, padded to a multiple of four
template <class W>
int64_t padded_block_sum(int64_t nrows, W&& width) {
  const int64_t nblocks = (nrows + kRB - 1) / kRB;
  return parallel_sums<1>(nblocks, [&](int64_t b0, int64_t b1, std::array<int64_t, 1>& mine) {
    for (int64_t b = b0; b < b1; ++b) {
      int64_t w = 0;
      for (int64_t r = b * kRB; r < std::min(nrows, (b + 1) * kRB); ++r) w = std::max<int64_t>(w, width(r));
      mine[0] += ((w + 3) & ~(int64_t)3) * kRB;
    }
  }, 1024)[0];
}

// the blocks outside [W0, R1): what a walk leaves to the per-block path
std::vector<int32_t> edge_blocks(int64_t W0, int64_t R1, int64_t nblocks) {
  std::vector<int32_t> edge;
  for (int64_t idx = 0; idx < W0 + (nblocks - R1); ++idx) edge.push_back((int32_t)qp::walk_edge_block(W0, R1, idx));
  return edge;
}

// rows i = a g + c strip by strip: `sw` consecutive inner indices c, all outer indices a in turn; fn(a, c) for every cell of
// step x step rows that lies inside its strip and inside the na outer indices
template <class F>
void for_each_strip_cell(int64_t g, int64_t sw, int64_t na, int64_t step, F&& fn) {
  for (int64_t c0 = 0; c0 < g; c0 += sw)
    for (int64_t a = 0; a + step - 1 < na; a += step)
      for (int64_t c = c0; c + step - 1 < std::min(c0 + sw, g); c += step) fn(a, c);
}

std::string reason_text(const char* fmt, long long a = 0, long long b = 0) {
  char buf[200];
  std::snprintf(buf, sizeof buf, fmt, a, b);
  return buf;
}

// the fullest row near the middle of the matrix (the middle row itself may sit on a grid's edge): the 256 rows around it;
// `wide`: and rows further out
int64_t fullest_middle_row(const UnionPattern& A, bool wide) {
  const int64_t n = A.nrows;
  int64_t rm = n / 2;
  auto probe = [&](int64_t r) {
    if (r >= 0 && r < n && row_len(A, r) > row_len(A, rm)) rm = r;
  };
  for (int64_t r = std::max<int64_t>(0, n / 2 - 128); r < std::min(n, n / 2 + 128); ++r) probe(r);
  if (!wide) return rm;
  for (int64_t t = -32; t <= 32; ++t) probe(n / 2 + t * 4099);   // (a whole line of a three-dimensional grid may sit on an edge: look further out too)
  // (... or a whole band of planes, when the stencil reaches two lines and two planes out and the grid is small: 2048 rows
  // spread over the middle half, at offsets that run through every position inside a line)
  for (int64_t k = 0; k < 2048; ++k) probe(n / 4 + (k * (n / 2)) / 2048 + (k * 37) % 64);
  return rm;
}

}  // namespace

int walk_shape_reason(const std::vector<int64_t>& dl, WalkShape& w, std::string* why) {
  auto say = [&](const char* fmt, long long a = 0, long long b = 0) {
    if (why) *why = reason_text(fmt, a, b);
  };
  const int z = (int)dl.size();
  if (z < 3 || z > 19) {
    say("%lld entries per row (the walk takes 3 to 19)", z);
    return QP_WALK_ROW_LENGTH;
  }
  for (int k = 0; k < z; ++k)
    if (dl[(size_t)k] != -dl[(size_t)(z - 1 - k)]) {   // mirror images of each other
      say("column distance %lld has no mirror image %lld in the row", dl[(size_t)k], -dl[(size_t)k]);
      return QP_WALK_NOT_MIRRORED;
    }
  int nbig = 0;
  while (nbig < z && dl[(size_t)nbig] <= -(int64_t)kRB) ++nbig;
  if (nbig < 1) {
    say("no column distance of at least 64 rows: a band of half-width %lld has no strip step", -dl[0]);
    return QP_WALK_NO_FAR;
  }
  // near part first: it decides between "too many / too far near" and the far diagnoses below
  {
    int k = nbig, nnear = 0;
    while (k < z && dl[(size_t)k] < 0) ++k, ++nnear;
    if (nnear >= 1 && -dl[(size_t)nbig] > qp::kWalkHalo) {
      say("near column distance %lld exceeds the %lld-row halo of the walk's window", -dl[(size_t)nbig], qp::kWalkHalo);
      return QP_WALK_NEAR_TOO_FAR;
    }
    if (nnear > 4) {
      say("%lld near column distances per side (the walk takes 1 to 4)", nnear);
      return QP_WALK_TOO_MANY_NEAR;
    }
    if (nnear < 1) {
      say("no near column distance (the walk's kernels take 1 to 4 within %lld rows)", qp::kWalkHalo);
      return QP_WALK_NO_NEAR;
    }
  }
  if (nbig > 6) {
    say("%lld far column distances per side (the walk takes up to 4 multiples of one stride, or up to 2 plus one or two long pairs)", nbig);
    return QP_WALK_TOO_MANY_FAR;
  }
  w = WalkShape();
  w.g = -dl[(size_t)(nbig - 1)];
  auto multiples = [&](int first, int K) {
    for (int m = 1; m <= K; ++m)
      if (dl[(size_t)(first + K - m)] != -(int64_t)m * w.g) return false;
    return true;
  };
  if (nbig == 3 && dl[0] + 1 == dl[1] && dl[1] + 1 == dl[2] && -dl[2] >= (int64_t)kRB) {
    // -(g + 1), -g, -(g - 1): one strip step with its two diagonal neighbours (the nine-point stencil of a two-dimensional grid)
    w.g = -dl[1];
    w.K = 1;
    w.fd = 1;
  } else if (nbig == 4 && dl[1] + 1 == dl[2] && dl[2] + 1 == dl[3] && -dl[3] >= (int64_t)kRB && -dl[0] > -dl[1] + qp::kWalkHalo) {
    // ... and one long pair beyond them: layers of such planes (+-nx ny)
    w.g = -dl[2];
    w.K = 1;
    w.fd = 1;
    w.xl = 1;
    w.glong = -dl[0];
  } else if (nbig <= 4 && multiples(0, nbig)) {
    w.K = nbig;
  } else if (nbig >= 2 && nbig <= 5 && multiples(1, nbig - 1) && -dl[0] > (int64_t)(nbig - 1) * w.g) {
    w.K = nbig - 1;
    w.xl = 1;
    w.glong = -dl[0];
  } else if (nbig >= 3 && multiples(2, nbig - 2) && -dl[1] > (int64_t)(nbig - 2) * w.g) {   // (sorted: -dl[0] > -dl[1])
    w.K = nbig - 2;
    w.xl = 2;
    w.glong = -dl[0];
    w.glong1 = -dl[1];
  } else {
    long long bad = 0;
    for (int i = 0; i < nbig; ++i)
      if ((-dl[(size_t)i]) % w.g != 0) bad = -dl[(size_t)i];
    if (bad) say("far column distance %lld is no multiple of the strip step %lld (two incommensurate strides)", bad, w.g);
    else say("far column distances are multiples of %lld but not the consecutive ones 1 .. K, K <= 4 (largest: %lld)", w.g, -dl[0]);
    return bad ? QP_WALK_INCOMMENSURATE : QP_WALK_TOO_MANY_FAR;
  }
  int k = nbig;
  while (k < z && dl[(size_t)k] < 0) ++k, ++w.nn;
  for (int i = 0; i < w.nn; ++i) w.near[i] = (int)(-dl[(size_t)(nbig + w.nn - 1 - i)]);
  w.z0 = (k < z && dl[(size_t)k] == 0) ? 1 : 0;
  if (z != 2 * (w.nn + w.K * (1 + 2 * w.fd) + w.xl) + w.z0) {
    say("row of %lld entries does not split into diagonal + near + far parts", z);
    return QP_WALK_NOT_MIRRORED;
  }
  if (w.xl >= 1) {
    // a "long" distance right beside the ring's far reach is a DIAGONAL neighbour (nine-point stencil: g - 1, g, g + 1 read as
    // stride g - 1 plus two long pairs): its operands are lane shifts of the ring's elements, which the walk does not keep in
    // a window -- loading them directly makes the walk no faster than the per-block kernel (N = 2^22: 117.9 vs 113.9 us)
    const int64_t first = (w.xl == 2) ? w.glong1 : w.glong;
    if (first - (int64_t)w.K * w.g <= qp::kWalkHalo) {
      say("distance %lld is a diagonal neighbour of the far reach %lld (windows on the ring's far steps are not built; the per-block kernel is as fast)",
          first, (long long)w.K * w.g);
      return QP_WALK_NO_KERNEL;
    }
  }
  if (w.fd && !qp::walk_shape_supported(w.nn, w.K, w.z0, w.xl, w.fd)) {
    say("no kernel instance for %lld near distances beside diagonal far neighbours (they come with at most 2 near and one long pair)", w.nn);
    return QP_WALK_NO_KERNEL;
  }
  if (!w.fd && !qp::walk_shape_supported(w.nn, w.K, w.z0, w.xl)) {
    say("no kernel instance for %lld near and %lld far distances with long pairs (they come with at most 2 near, 2 far)", w.nn, w.K);
    return QP_WALK_NO_KERNEL;
  }
  return QP_WALK_OK;
}

// Strip-walk plan of a Hermitian-packed lattice operator (walk_geometry.h: WalkPlan; kernels_walk.hip).  Looks, in the union
// pattern itself, for the longest run of row blocks in which every row has the same list of column distances, checks that
// the list has the shape the walk needs -- [-K g .. -g] [-d_nn .. -d_1] [0]? [d_1 .. d_nn] [g .. K g], g a multiple of 64
// rows -- and that the upper values of the run's blocks lie at equal strides.  With one stencil on every row of the run the
// position of every value, and of every conj-transposed value, is a formula; how the column sections of those blocks are
// encoded does not matter (the walk reads none of them).  The remaining blocks are listed for the per-block path.
WalkPlans plan_walk(const UnionPattern& A, const HostLayout& Lh) {
  WalkPlans out;
  qp::WalkPlan& P = out.one;
  const int64_t nb = (A.nrows + kRB - 1) / kRB;
  auto why = [&](int code, const char* fmt, long long a = 0, long long b = 0) {
    out.reason = code;
    out.text = reason_text(fmt, a, b);
    return std::move(out);
  };
  if (Lh.format != QP_FMT_HRB) return why(QP_WALK_NOT_PACKED, "device format %lld is not the Hermitian-packed one", Lh.format);
  if (nb < 8 || A.ncols < A.nrows) return why(QP_WALK_TOO_FEW_BLOCKS, "%lld row blocks (or fewer columns than rows)", nb);   // (more columns than rows: the halo slabs of a row-partitioned operator)
  const int64_t nfull = A.nrows / kRB;   // (a partly filled last block never belongs to the run)
  // Longest run of row blocks whose rows all carry ONE list of column distances.  "Same distances" is transitive, so a block
  // belongs to the run of the block before it iff (a) its own 64 rows agree with one another and (b) its first row agrees with the
  // first row of the block before: both per block, on a few host threads; the runs are then read off the two flag arrays.
  std::vector<char> uniform((size_t)std::max<int64_t>(nfull, 1), 0), joins((size_t)std::max<int64_t>(nfull, 1), 0);
  parallel_rows(nfull, [&](int64_t b0, int64_t b1) {
    for (int64_t b = b0; b < b1; ++b) {
      const int64_t ref = b * kRB;
      const int64_t len = row_len(A, ref);
      bool ok = len >= 3 && len <= 19;
      for (int64_t r = ref + 1; r < ref + kRB && ok; ++r) ok = same_distances(A, r, ref);
      uniform[(size_t)b] = ok ? 1 : 0;
      joins[(size_t)b] = (ok && b > 0 && same_distances(A, ref, ref - kRB)) ? 1 : 0;
    }
  }, 1024);
  int64_t best0 = 0, best1 = 0;
  for (int64_t b = 0; b < nfull;) {
    if (!uniform[(size_t)b]) {
      ++b;
      continue;
    }
    int64_t e = b + 1;
    while (e < nfull && uniform[(size_t)e] && joins[(size_t)e]) ++e;
    if (e - b > best1 - best0) best0 = b, best1 = e;
    b = e;
  }
  if (best1 - best0 < 8)
    return why(QP_WALK_NO_UNIFORM_RUN, "the longest run of row blocks whose rows all carry one list of column distances is %lld blocks (of %lld): not a lattice",
               best1 - best0, nb);
  const int64_t R0 = best0, R1 = best1, rref = R0 * kRB;
  WalkShape ws;
  out.reason = walk_shape_reason(row_distances(A, rref), ws, &out.text);
  if (out.reason != QP_WALK_OK) return out;
  const int nn = ws.nn, K = ws.K, z0 = ws.z0, xl = ws.xl, fd = ws.fd, KF = ws.K * (1 + 2 * ws.fd);
  const int64_t g = ws.g;
  for (int i = 0; i < nn; ++i) P.near[i] = ws.near[i];
  const int S = (int)((g + kRB - 1) / kRB);
  // first block whose rows find their history (K g rows back, L for the long pair) inside the run
  const int64_t W0 = R0 + (std::max<int64_t>((int64_t)K * g + fd, ws.glong) + kRB - 1) / kRB;
  if (R1 - W0 < 8) return why(QP_WALK_TOO_FEW_BLOCKS, "%lld walkable row blocks after the first %lld of the run (whose history lies outside it)", R1 - W0, W0 - R0);
  // the upper section of every block of the run: z0 + nn + K entries per row, padded to a multiple of four, at equal strides
  const int64_t wu = ((z0 + nn + KF + xl + 3) / 4) * 4;
  const int64_t U0 = Lh.bptr[R0], ustride = wu * kRB;
  for (int64_t b = R0; b <= R1; ++b)
    if (Lh.bptr[b] != U0 + (b - R0) * ustride) return why(QP_WALK_LAYOUT, "upper sections of the run are not at equal strides (block %lld)", b);
  for (int64_t r = rref; r < R1 * kRB; r += kRB)
    if (Lh.nlow[r] != nn + KF + xl) return why(QP_WALK_LAYOUT, "row %lld has %lld lower entries", r, Lh.nlow[r]);
  if (U0 + (R1 - R0) * ustride >= (int64_t)INT32_MAX) return why(QP_WALK_LAYOUT, "value positions beyond 2^31");
  out.edge = edge_blocks(W0, R1, nb);
  P.nn = nn;
  P.K = K;
  P.z0 = z0;
  P.S = S;
  P.g = g;
  P.xl = xl;
  P.glong = ws.glong;
  P.glong1 = ws.glong1;
  P.fd = fd;
  P.R0 = R0;
  P.R1 = R1;
  P.W0 = W0;
  P.U0 = U0;
  P.ustride = (int)ustride;
  P.n_edge = (int64_t)out.edge.size();
  P.valid = 1;
  // the two-term walk's plan: the region in which phase Z (term m + 1 of block t - K) finds y of the K blocks on either side formed
  // by the same walk -- [W0 + K S, R1 - K S) -- and, as its edge list, every block outside it (they take two per-block launches)
  if (!xl && !fd && g % kRB == 0 && qp::walk2_shape_supported(nn, K, z0) && (R1 - W0) - 2 * (int64_t)K * S >= 8 * (int64_t)S) {
    qp::WalkPlan& Q = out.two;
    Q = P;
    Q.W0 = W0 + (int64_t)K * S;
    Q.R1 = R1 - (int64_t)K * S;
    out.edge2 = edge_blocks(Q.W0, Q.R1, nb);
    Q.n_edge = (int64_t)out.edge2.size();
  }
  return out;
}

// Column-blocked mirror (device.h: ColBlockPlan; kernels_colblock.hip) for an operator whose gathers are irregular.
// Decision (knob colblock = 1): plain row blocks or CSR (a lattice is Hermitian-packed and walked; a dense operator has
// its own kernels), at least 2^20 (kCbMinLog2N) columns (below, the vector sits in the L2 as it is), at most 64 column blocks
// and kCbMaxTilesPerWave tiles per resident wavefront of a chip of `cu` compute units, and -- sampled over the row blocks -- more
// than half of the gathers of a wavefront's load pulling a 128-byte line of their own (a band or a lattice shares each line among
// 8 lanes: 0.125).
ColBlockHost plan_colblock(const UnionPattern& A, const HostLayout& L, const PlanKnobs& tun, int cu) {
  ColBlockHost out;
  if (tun.colblock == 0 || (L.format != QP_FMT_RBCSR && L.format != QP_FMT_CSR)) return out;
  const auto& ur = A.ur;
  const auto& uc = A.uc;
  const int64_t nrows = A.nrows, ncols = A.ncols, nnz = ur[nrows];
  if (nrows < 64 || nnz < 1 || nnz >= (int64_t)INT32_MAX || ncols >= ((int64_t)1 << 32)) return out;
  // columns per block: about sixteen blocks (measured, 16 random columns per row: N = 2^20 171 / 178 / 195 us per term with
  // 2^16 / 2^17 / 2^18 columns per block, 2^21 416 / 353 / 460, 2^22 1125 / 890 / 829 -- profiles/r04/colblock.txt), a block
  // never larger than half an XCD's L2 share would like (2^18 elements = 4 MB is the whole L2; taken only from 2^22 columns on)
  int log2w = tun.cb_log2w;
  if (log2w <= 0) {
    int lg = 0;
    while (((int64_t)1 << lg) < ncols) ++lg;
    log2w = std::max(16, std::min(lg - 4, 18));
  }
  log2w = std::max(6, std::min(log2w, 24));
  const int64_t W = (int64_t)1 << log2w;
  const int64_t P = (ncols + W - 1) / W;
  if (tun.colblock == 1 && (ncols < ((int64_t)1 << qp::kCbMinLog2N) || P < 2)) return out;
  if (P > 256) return out;
  // irregularity: distinct 128-byte lines among the k-th gathers of a 64-row block, over the entries sampled
  {
    const int64_t nblocks = nrows / kRB;
    const int64_t bstride = std::max<int64_t>(1, nblocks / 1024);
    int64_t gathers = 0, lines = 0, local = 0;
    std::vector<int64_t> ln;
    for (int64_t b = 0; b < nblocks; b += bstride) {
      int64_t wmax = 0;
      for (int64_t r = b * kRB; r < (b + 1) * kRB; ++r) wmax = std::max(wmax, row_len(A, r));
      for (int64_t k = 0; k < wmax; ++k) {
        ln.clear();
        for (int64_t r = b * kRB; r < (b + 1) * kRB; ++r)
          if (k < row_len(A, r)) {
            const int64_t c = uc[ur[r] + k];
            ln.push_back(c >> 3);
            if (std::llabs(c - r) <= ((int64_t)1 << 16)) ++local;
          }
        std::sort(ln.begin(), ln.end());
        gathers += (int64_t)ln.size();
        lines += (int64_t)(std::unique(ln.begin(), ln.end()) - ln.begin());
      }
    }
    out.line_share = gathers > 0 ? (double)lines / (double)gathers : 0.0;
    if (tun.colblock == 1 && out.line_share <= 0.5) return out;
    // ... and the gathers must really leave the L2: columns drawn near the row (within 2^16 elements = 1 MB either side)
    // stay in the XCD's L2 as the rows stream by -- columns random inside 4096-row windows: 101 us per term on the
    // row-block kernel, 186 through the mirror
    if (tun.colblock == 1 && 4 * local >= 3 * gathers) return out;
  }
  // tile height: 128 rows unless a segment would outgrow the wavefront's LDS buffer, then 64
  std::vector<int32_t> segcnt;
  int rpt = 0, max_seg = 0;
  int64_t ntiles = 0;
  for (int tryr : {2, 1}) {
    const int64_t TR = 64 * tryr;
    ntiles = (nrows + TR - 1) / TR;
    segcnt.assign((size_t)(ntiles * P + 1), 0);
    parallel_rows(ntiles, [&](int64_t t0, int64_t t1) {
      for (int64_t t = t0; t < t1; ++t)
        for (int64_t r = t * TR; r < std::min(nrows, (t + 1) * TR); ++r)
          for (int64_t p = ur[r]; p < ur[r + 1]; ++p) segcnt[(size_t)(t * P + ((int64_t)uc[p] >> log2w))]++;
    }, 512);
    max_seg = 0;
    for (int64_t sgi = 0; sgi < ntiles * P; ++sgi) max_seg = std::max(max_seg, (int)segcnt[(size_t)sgi]);
    if (max_seg <= qp::kCbMaxSeg) {
      rpt = tryr;
      break;
    }
  }
  if (rpt == 0) return out;   // a (64-row, 2^log2w-column) cell with more than kCbMaxSeg entries: not this kernel's operator
  {
    const int64_t resident = (int64_t)std::max(cu, 1) * qp::kCbWavesPerCu;
    if ((ntiles + resident - 1) / resident > qp::kCbMaxTilesPerWave) return out;
  }
  const int64_t TR = 64 * rpt;
  std::vector<int32_t>& segptr = out.segptr;
  segptr.resize((size_t)(ntiles * P + 1));
  {
    int64_t run = 0;
    for (int64_t sgi = 0; sgi < ntiles * P; ++sgi) {
      segptr[(size_t)sgi] = (int32_t)run;
      run += segcnt[(size_t)sgi];
    }
    segptr[(size_t)(ntiles * P)] = (int32_t)run;
  }
  std::vector<int64_t> vmap;
  csr_value_map(L, nrows, ur, uc, vmap);
  std::vector<uint16_t>& rowoff = out.rowoff;
  std::vector<uint32_t>& cols = out.cols;
  std::vector<int64_t>& map = out.map;
  rowoff.resize((size_t)(ntiles * P) * (size_t)(TR + 1));
  cols.resize((size_t)nnz);
  map.resize((size_t)nnz);
  parallel_rows(ntiles, [&](int64_t t0, int64_t t1) {
    std::vector<int32_t> fill((size_t)P);
    for (int64_t t = t0; t < t1; ++t) {
      for (int64_t c = 0; c < P; ++c) fill[(size_t)c] = 0;
      for (int64_t l = 0; l < TR; ++l) {
        const int64_t r = t * TR + l;
        for (int64_t c = 0; c < P; ++c) rowoff[(size_t)(t * P + c) * (size_t)(TR + 1) + (size_t)l] = (uint16_t)fill[(size_t)c];
        if (r >= nrows) continue;
        for (int64_t p = ur[r]; p < ur[r + 1]; ++p) {
          const int64_t c = (int64_t)uc[p] >> log2w;
          const int64_t e = (int64_t)segptr[(size_t)(t * P + c)] + fill[(size_t)c]++;
          cols[(size_t)e] = (uint32_t)uc[p];
          map[(size_t)e] = vmap[(size_t)p];
        }
      }
      for (int64_t c = 0; c < P; ++c) rowoff[(size_t)(t * P + c) * (size_t)(TR + 1) + (size_t)TR] = (uint16_t)fill[(size_t)c];
    }
  }, 512);
  out.shape.log2w = log2w;
  out.shape.P = (int)P;
  out.shape.rpt = rpt;
  out.shape.max_seg = max_seg;
  out.shape.ntiles = ntiles;
  out.shape.nnz = nnz;
  out.shape.valid = 1;
  return out;
}

int choose_format(const UnionPattern& A, int requested, bool hermitian, const PlanKnobs& tun) {
  if (requested != QP_FMT_AUTO) return (requested == QP_FMT_HRB && !hermitian) ? -1 : requested;
  const auto& ur = A.ur;
  const auto& uc = A.uc;
  const int64_t nrows = A.nrows, nnz = ur[nrows];
  const int64_t nblocks = (nrows + kRB - 1) / kRB;
  const int64_t rb_stored = padded_block_sum(nrows, [&](int64_t r) { return row_len(A, r); });
  // the row-block kernels stream ~1.6x faster than the sub-wave CSR kernel at equal bytes
  // (profiles/r01/kbench_*): accept up to 50 % padding before falling back
  const bool rb_ok = (double)rb_stored <= 1.5 * (double)nnz + 1024.0;
  // (a Hermitian operator is judged by the padding of its packed form further down: five entries per row -- the
  // five-point lattice -- pad to eight as plain row blocks, but to four upper entries when packed)
  if (!rb_ok && !hermitian) return QP_FMT_CSR;
  // few, long rows (small dense generators: the reference's test and benchmark sizes): a
  // row block gives one wavefront 64 rows to walk entry by entry -- too few wavefronts to
  // hide the latency.  One wavefront per row instead (CSR kernel, 64 lanes per row).
  if (nblocks < 2048 && nnz >= 32 * nrows) return QP_FMT_CSR;
  if (!hermitian) return QP_FMT_RBCSR;
  // values the packed form stores: the upper section of every block, padded to a multiple of four
  const int64_t hu_stored = padded_block_sum(nrows, [&](int64_t r) {
    const int32_t* cb = uc.data() + ur[r];
    const int32_t* ce = uc.data() + ur[r + 1];
    return (int64_t)(ce - std::lower_bound(cb, ce, (int32_t)r));
  });
  const bool hrb_ok = rb_ok || (double)hu_stored <= 0.9 * (double)nnz + 1024.0;
  // Hermitian packing pays only if the transposed values are still in the XCD's L2
  // (4 MiB) when the lower entry is processed: the rows stream in order, so require
  // (row - col) * bytes-per-row <= 2 MiB for at least 85 % of the lower entries.
  // Measured (profiles/r01/kbench): banded 53.6 vs 72.1 us per term, scattered 103.8 vs 93.4.
  const double row_bytes = 14.0 * (double)nnz / (double)std::max<int64_t>(nrows, 1) + 80.0;
  const int64_t maxdist = (int64_t)(2.0 * 1048576.0 / row_bytes);
  const auto low = parallel_sums<2>(nrows, [&](int64_t r0, int64_t r1, std::array<int64_t, 2>& mine) {
    for (int64_t r = r0; r < r1; ++r)
      for (int64_t p = ur[r]; p < ur[r + 1] && uc[p] < r; ++p) {
        ++mine[0];
        if (r - uc[p] <= maxdist) ++mine[1];
      }
  });
  const int64_t nlow = low[0], nnear = low[1];
  // ... and only if the transposed reads are coalesced: in a block whose 64 rows have their k-th entry at
  // the same distance from the diagonal (stencil-like: lattices, tensor products) the wave reads 64
  // consecutive values; in an irregular block every lane pulls its own L2 line for 16 useful bytes
  // (measured, columns drawn per row inside 4096-row windows: Hermitian-packed 138 us vs 103 us per
  // term, profiles/r02/kbench_random_window.txt).  A sample of the blocks decides: the lower entries (col < row: the ones read
  // through the transposed position) of every row of the block at the same distances from the diagonal
  int64_t sampled = 0, regular = 0;
  const int64_t bstride = std::max<int64_t>(1, nblocks / 512);
  for (int64_t b = 0; b < nblocks; b += bstride) {
    const int64_t r0 = b * kRB, r1 = std::min(nrows, r0 + kRB);
    if (r1 - r0 < kRB) continue;
    ++sampled;
    bool same = true;
    for (int64_t r = r0 + 1; r < r1 && same; ++r) same = same_distances(A, r, r0, true);
    if (same) ++regular;
  }
  const bool coalesced = sampled == 0 || 4 * regular >= 3 * sampled;
  // (the packed format addresses the transposed values with int32 positions)
  // ... unless the operator will take the strip walk, which reads a far transposed value one step ahead like any other
  // stream instead of waiting for it in the row sum (the plane distance of a three-dimensional grid is 32768 rows away:
  // 256 x 128 x 128 grid 136 us per term as plain row blocks, 101 packed and walked)
  bool walkable = false;
  if (tun.hrb_walk && nblocks >= tun.walk_min_blocks) {
    WalkShape wsh;
    walkable = parse_walk_shape(row_distances(A, fullest_middle_row(A, false)), wsh) && 4 * regular >= 3 * sampled;
  }
  if (((double)nnear >= 0.85 * (double)nlow || walkable) && coalesced && hrb_ok && rb_stored < (int64_t)INT32_MAX) return QP_FMT_HRB;
  return rb_ok ? QP_FMT_RBCSR : QP_FMT_CSR;
}

// Lattice completion (knob lattice_fill).  A finite-difference operator on an nx x ny grid with open boundaries is the
// walk's lattice -- distances +-1, +-nx -- except that the rows at x = 0 lack the -1 entry and those at x = nx - 1 the +1
// entry: one row in nx breaks the "same distances on every row" run that the strip walk (and the stencil encoding of the
// row blocks) needs.  If every row between the first and the last K g rows carries a SUBSET of the middle row's distance
// list, that list has the walk's shape, and at most 12 % of the entries are missing (a 64 x 8 x nz grid: 4 %), the missing ones are stored as explicit
// zeros (with their transposes, so that the pattern stays structurally symmetric).  Index work only; 0 * x terms change no
// row sum beyond the order in which the two accumulators of a row take their entries.
void lattice_fill(const PlanKnobs& tun, int64_t n, int64_t ncols, UnionRowptr& ur, UnionCols& uc, UnionRowptr* ur_before,
                  UnionCols* uc_before) {
  if (!tun.lattice_fill || ncols < n || n / kRB < std::max(tun.walk_min_blocks, 16)) return;
  // (ncols > n: the local rows of a row-partitioned operator; its halo columns appear only in the first / last K g rows)
  const UnionPattern A{n, ncols, ur, uc};
  const std::vector<int64_t> D = row_distances(A, fullest_middle_row(A, true));   // the reference row
  const int z = (int)D.size();
  if (z < 3 || z > 19) return;
  WalkShape ws;
  if (!parse_walk_shape(D, ws)) return;
  const int64_t reach = std::max<int64_t>((int64_t)ws.K * ws.g + ws.fd, ws.glong);
  const int64_t lo = reach, hi = n - reach;
  if (hi - lo < 16 * (int64_t)kRB) return;
  int64_t missing = 0;
  {   // nothing to complete when every row between lo and hi already has z entries (the headline lattice): skip the check
    bool longer = false;
    for (int64_t r = lo; r < hi && !longer; ++r) {
      const int64_t len = ur[r + 1] - ur[r];
      longer = len > z;
      missing += z - len;
    }
    if (longer || missing == 0) return;
    missing = 0;
  }
  for (int64_t r = lo; r < hi; ++r) {
    int d = 0;
    for (int64_t p = ur[r]; p < ur[r + 1]; ++p) {
      if (uc[p] >= n) return;
      const int64_t delta = (int64_t)uc[p] - r;
      while (d < z && D[(size_t)d] < delta) ++d;
      if (d == z || D[(size_t)d] != delta) return;   // an entry outside the lattice's distances: not this kind of operator
      ++d;
    }
    missing += z - (ur[r + 1] - ur[r]);
  }
  if (missing == 0 || (double)missing > 0.12 * (double)ur[n]) return;
  // transposes of filled entries that land in the first / last K g rows
  std::vector<std::pair<int64_t, int32_t>> extra;
  for (int64_t r = lo; r < hi; ++r) {
    if (ur[r + 1] - ur[r] == z) continue;
    int64_t p = ur[r];
    for (int d = 0; d < z; ++d) {
      const int64_t c = r + D[(size_t)d];
      if (p < ur[r + 1] && uc[p] == c) {
        ++p;
        continue;
      }
      if (c < lo || c >= hi) extra.emplace_back(c, (int32_t)r);
    }
  }
  std::sort(extra.begin(), extra.end());
  UnionRowptr nr((size_t)n + 1, 0);
  UnionCols nc;
  nc.reserve(uc.size() + (size_t)missing + extra.size());
  size_t ex = 0;
  std::vector<int32_t> row;
  for (int64_t r = 0; r < n; ++r) {
    if (r >= lo && r < hi) {
      for (int d = 0; d < z; ++d) nc.push_back((int32_t)(r + D[(size_t)d]));
    } else {
      row.assign(uc.begin() + ur[r], uc.begin() + ur[r + 1]);
      while (ex < extra.size() && extra[ex].first == r) row.push_back(extra[ex++].second);
      std::sort(row.begin(), row.end());
      row.erase(std::unique(row.begin(), row.end()), row.end());
      nc.insert(nc.end(), row.begin(), row.end());
    }
    nr[(size_t)r + 1] = (int64_t)nc.size();
  }
  ur.swap(nr);
  uc.swap(nc);
  // the pattern as it was (the caller takes the completion back when the operator does not end up walked) -- handed over only
  // when something was completed: no copy of a pattern that stays as it is
  if (ur_before) ur_before->swap(nr);
  if (uc_before) uc_before->swap(nc);
}

// ---- plans of the batched path (qp_cheby_step_batched): the row walk of the row kernel and the LDS-staged tiles ----
// Row walk for the batched kernel (kernels_spmm.hip: spmm_rows_kernel).  The pattern is
// sampled for its offsets d = col - row (folded to (-n/2, n/2]); when the far ones (|d| >= 64) are all
// multiples of one inner dimension g -- H = H_a (x) 1 + 1 (x) H_c, i = a g + c: lattice and tensor-product
// operators -- the rows are listed strip by strip: `sw` consecutive inner indices c, all outer indices a
// in turn.  Then the rows that gather a given row of X (its +-k g and +-near neighbours) are visited
// within a few strip widths of each other instead of 2 a_max g rows apart, and the strip width is chosen
// so that this window, plus the rows in flight, fits half an XCD's L2 at `batch` states per row.
// Anything else (no far offsets, no common inner dimension, strips narrower than four times the near
// reach) keeps the natural order.  Index work only: the arithmetic per row does not change.
SpmmOrder plan_spmm_order(const UnionPattern& A, int batch, int knob) {
  SpmmOrder out;
  const int64_t n = A.nrows;
  if (knob < 0 || n < 4096 || n > INT32_MAX || A.ncols != n || A.ur.empty()) return out;
  int64_t g = 0, far_max = 0, near_max = 0;
  const int64_t nsample = std::min<int64_t>(n, 4096), stride = n / nsample;
  for (int64_t t = 0; t < nsample; ++t)
    for (int64_t d : row_distances(A, t * stride, true)) {
      d = std::llabs(d);
      if (d >= 64) {
        g = std::gcd(g, d);
        far_max = std::max(far_max, d);
      } else {
        near_max = std::max(near_max, d);
      }
    }
  if (g < 256 || far_max / g > 64) return out;
  const int64_t amax = far_max / g;
  const int64_t l2_budget = 1280 * 1024;                 // under a third of an XCD's 4 MiB L2 for the gather window (measured at
                                                         // 64 states: strips of 64 beat 128 and 32, profiles/r02/batched_c5_sweep.txt)
  const int64_t row_bytes = (int64_t)std::min(batch, 64) * 16;   // (16 bytes per state)
  int64_t sw;
  if (knob > 0) {
    sw = knob;
  } else {
    const int64_t inflight = 512;                         // rows an XCD has in flight (32 CUs x 16 waves)
    sw = (l2_budget / row_bytes - inflight) / (2 * amax + 1);
  }
  sw = std::min(sw, g);
  while (sw > 1 && g % sw != 0) --sw;                     // every strip the same width
  if (sw < 1) return out;
  if (knob == 0 && (sw < 4 * std::max<int64_t>(near_max, 1) || sw < 16)) return out;
  if (sw >= g) return out;                                // one strip = the natural order
  out.order.resize((size_t)n);
  size_t k = 0;
  for_each_strip_cell(g, sw, (n + g - 1) / g, 1, [&](int64_t a, int64_t c) {
    const int64_t i = a * g + c;
    if (i < n) out.order[k++] = (int32_t)i;
  });
  if ((int64_t)k != n) {   // cannot happen; fall back to the natural order rather than skip rows
    out.order.clear();
    return out;
  }
  out.g = g;
  out.sw = sw;
  return out;
}

// Tiles of the batched path (device.h: SpmmTiles; kernel: spmm_tile_kernel).  The pattern of the row in the middle of the matrix is
// the candidate: every distance near (|d| <= 4) or a multiple m g of the far distances' gcd with |m| <= 4.  A row is regular when
// its entries are exactly that pattern; a tile is sixteen regular rows r0 + i g + j (i, j < 4, r0 = 4 ta g + 4 tc).  Tiles are
// listed strip by strip like the row walk above (the kernel is not sensitive to the strip width: any order that keeps the tiles of
// neighbouring strip steps close in time serves the far halo from L2); every other row goes to the row kernel.  Index work only.
SpmmTilesHost plan_spmm_tiles(const UnionPattern& A, int knob) {
  SpmmTilesHost out;
  const int64_t n = A.nrows;
  if (knob < 0 || n < 4096 || n > INT32_MAX || A.ncols != n || A.ur.empty() || A.ur[n] > (int64_t)INT32_MAX) return out;
  const int64_t rm = n / 2;
  const std::vector<int64_t> D = row_distances(A, rm);
  const int nd = (int)D.size();
  if (nd < 2 || nd > qp::kSpmmTileMaxEntries) return out;
  int64_t g = 0, far_max = 0, near_max = 0;
  for (int64_t d : D) {
    const int64_t ad = std::llabs(d);
    if (ad <= 4) near_max = std::max(near_max, ad);
    else if (ad >= 64) {
      g = std::gcd(g, ad);
      far_max = std::max(far_max, ad);
    } else return out;
  }
  if (g < 64 || far_max / g > 4) return out;
  qp::SpmmTileShape sh;
  sh.nd = nd;
  sh.K = (int)(far_max / g);
  sh.NN = (int)near_max;
  for (int k = 0; k < nd; ++k) {
    const int64_t d = D[(size_t)k];
    const bool nearby = std::llabs(d) <= 4 && d != 0;
    sh.dnear[k] = nearby ? (int)d : 0;
    sh.dfar[k] = nearby ? 0 : (int)(d / g);
  }
  std::vector<uint8_t> regular((size_t)n);
  parallel_rows(n, [&](int64_t r_begin, int64_t r_end) {
    for (int64_t r = r_begin; r < r_end; ++r) regular[(size_t)r] = same_distances(A, r, rm) ? 1 : 0;
  });
  int64_t sw = knob > 0 ? knob : 128;
  sw = std::max<int64_t>(4, std::min(sw, g) / 4 * 4);
  std::vector<uint8_t> covered((size_t)n, 0);
  for_each_strip_cell(g, sw, (n + g - 1) / g, 4, [&](int64_t a0, int64_t c) {
    const int64_t r0 = a0 * g + c;
    if (r0 + 3 * g + 3 >= n) return;
    bool ok = true;
    for (int i = 0; ok && i < 4; ++i)
      for (int j = 0; ok && j < 4; ++j) ok = regular[(size_t)(r0 + i * g + j)] != 0;
    if (!ok) return;
    out.tiles.push_back((int32_t)r0);
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) covered[(size_t)(r0 + i * g + j)] = 1;
  });
  if ((int64_t)out.tiles.size() * 16 < n / 2) {   // mostly edges: the row kernel alone
    out.tiles.clear();
    return out;
  }
  for (int64_t r = 0; r < n; ++r)
    if (!covered[(size_t)r]) out.rest.push_back((int32_t)r);
  out.shape = sh;
  out.g = g;
  out.sw = sw;
  return out;
}

// the tile kernel's table: where the staged rows lie relative to r0, where every wavefront finds its operands in LDS
SpmmTileTable spmm_tile_table(const qp::SpmmTileShape& shape, int64_t g) {
  SpmmTileTable out;
  const int K = shape.K, NN = shape.NN, nfar = (4 + 2 * K) * 4;
  out.T = nfar + 8 * NN;
  std::vector<int32_t>& tab = out.tab;
  tab.assign((size_t)qp::kSpmmTileTab, 0);
  for (int slot = 0; slot < out.T; ++slot) {
    int64_t d;
    if (slot < nfar) {
      d = (int64_t)(slot / 4 - K) * g + slot % 4;
    } else {
      const int s2 = slot - nfar, ii = s2 / (2 * NN), jj = s2 % (2 * NN);
      d = (int64_t)ii * g + (jj < NN ? jj - NN : 4 + jj - NN);
    }
    tab[(size_t)slot] = (int32_t)d;
  }
  for (int w = 0; w < 16; ++w) {
    const int i = w / 4, j = w % 4, own = (i + K) * 4 + j;
    for (int k = 0; k < shape.nd; ++k) {
      int slot;
      const int dn = shape.dnear[k];
      if (dn == 0) {
        slot = own + 4 * shape.dfar[k];
      } else {
        const int jj = j + dn;
        slot = (jj >= 0 && jj < 4) ? own + dn : nfar + i * 2 * NN + (jj < 0 ? jj + NN : jj - 4 + NN);
      }
      tab[(size_t)(qp::kSpmmTileSlots + qp::kSpmmTileMaxEntries * w + k)] = slot * qp::kSpmmTileRowBytes;
    }
    tab[(size_t)(qp::kSpmmTileSlots + qp::kSpmmTileMaxEntries * 16 + w)] = (int32_t)((int64_t)i * g + j);
    tab[(size_t)(qp::kSpmmTileSlots + qp::kSpmmTileMaxEntries * 16 + 16 + w)] = own * qp::kSpmmTileRowBytes;
  }
  return out;
}
