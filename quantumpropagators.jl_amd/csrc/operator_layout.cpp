// Host index work of the operator layouts (operator_layout.h): bit patterns and positions, no arithmetic on values beyond the
// summing of duplicate entries.  No HIP.
#include "operator_layout.h"

#include <atomic>
#include <unordered_map>

// ---- union pattern and the terms' values in its order -------------------------------------------------------------
// (one term whose rows are strictly ascending IS the union pattern; a term with repeated or unsorted columns goes through the
// merge like several terms do, so that density, completeness and every layout decision see each position once --
// a duplicate could make the stored count reach nrows x ncols with positions missing)
bool union_pattern(const std::vector<TermCsr>& terms, int64_t nrows, UnionRowptr& ur, UnionCols& uc) {
  bool canonical = terms.size() == 1;
  if (canonical) {
    const TermCsr& t = terms[0];
    std::atomic<bool> asc{true};
    parallel_rows(nrows, [&](int64_t r0, int64_t r1) {
      for (int64_t r = r0; r < r1 && asc.load(std::memory_order_relaxed); ++r)
        for (int64_t p = t.rowptr[r] + 1; p < t.rowptr[r + 1]; ++p)
          if (t.col[p] <= t.col[p - 1]) {
            asc.store(false, std::memory_order_relaxed);
            break;
          }
    });
    canonical = asc.load();
  }
  if (canonical) {
    ur.resize(terms[0].rowptr.size());
    uc.resize(terms[0].col.size());
    parallel_copy(ur.data(), terms[0].rowptr.data(), ur.size());
    parallel_copy(uc.data(), terms[0].col.data(), uc.size());
    return true;
  }
  ur.assign(nrows + 1, 0);
  std::vector<int32_t> merged;
  for (int64_t r = 0; r < nrows; ++r) {
    merged.clear();
    for (const TermCsr& t : terms) merged.insert(merged.end(), t.col.begin() + t.rowptr[r], t.col.begin() + t.rowptr[r + 1]);
    std::sort(merged.begin(), merged.end());
    merged.erase(std::unique(merged.begin(), merged.end()), merged.end());
    uc.insert(uc.end(), merged.begin(), merged.end());
    ur[r + 1] = (int64_t)uc.size();
  }
  return false;
}

void dense_complete(int64_t nrows, int64_t ncols, UnionRowptr& ur, UnionCols& uc) {
  if (ur[nrows] == nrows * ncols) return;
  uc.resize((size_t)(nrows * ncols));
  parallel_rows(nrows, [&](int64_t r0, int64_t r1) {
    for (int64_t r = r0; r < r1; ++r)
      for (int64_t c = 0; c < ncols; ++c) uc[(size_t)(r * ncols + c)] = (int32_t)c;
  });
  for (int64_t r = 0; r <= nrows; ++r) ur[r] = r * ncols;
}

void scatter_terms(const std::vector<TermCsr>& terms, bool canonical, int64_t nrows, const UnionRowptr& ur, const UnionCols& uc, Planes& planes) {
  const int64_t nnz = ur[nrows];
  auto same = [](const auto& a, const auto& b) {      // a == b, on the host threads (a gigabyte of columns at N = 2^24)
    if (a.size() != b.size()) return false;
    std::atomic<bool> eq{true};
    parallel_rows((int64_t)a.size(), [&](int64_t i0, int64_t i1) {
      if (i1 > i0 && std::memcmp(a.data() + i0, b.data() + i0, (size_t)(i1 - i0) * sizeof(a[0])) != 0) eq.store(false, std::memory_order_relaxed);
    }, (int64_t)1 << 20);
    return eq.load();
  };
  for (size_t l = 0; l < terms.size(); ++l) {
    const TermCsr& M = terms[l];
    auto& pv = planes[l];
    if (terms.size() == 1 && canonical && (int64_t)M.vals.size() == nnz && same(ur, M.rowptr) && same(uc, M.col)) {
      // one canonical term and no completion: the union pattern IS the term's own (same columns, not merely as many) -- a plain copy
      pv.borrow(M.vals);      // (the term outlives the operator build that reads it, nothing keeps the pointer)
      continue;
    }
    auto& o = pv.make_own((size_t)nnz);
    parallel_rows(nrows, [&](int64_t r0, int64_t r1) {
      for (int64_t r = r0; r < r1; ++r) {
        int64_t k = 0;
        for (int64_t p = M.rowptr[r]; p < M.rowptr[r + 1]; ++p) {
          while (uc[ur[r] + k] != M.col[p]) ++k;
          o[ur[r] + k] += M.vals[p];
        }
      }
    });
  }
}

// is this canonical CSR exactly Hermitian (bitwise conj-symmetric values, symmetric pattern, real diagonal, strictly increasing
// columns)?  Columns >= n (ghost columns of a row-partitioned operator in local numbering) are outside the square part and
// always carry their values.
bool csr_is_hermitian(int64_t n, const UnionRowptr& rp, const UnionCols& col, const PlaneView& vals) {
  // Every row on its own (rows in chunks on a few host threads): columns strictly ascending, a real diagonal, and for every
  // lower entry (r, c), c < r, the upper entry (c, r) with the conjugate value -- found by bisection in row c (rows are short);
  // as many lower entries as upper ones inside the square part then says that no upper entry lacks its partner.
  std::atomic<bool> ok{true};
  std::atomic<int64_t> nlower{0}, nupper{0};
  parallel_rows(n, [&](int64_t r_begin, int64_t r_end) {
    int64_t lo = 0, up = 0;
    for (int64_t r = r_begin; r < r_end && ok.load(std::memory_order_relaxed); ++r) {
      for (int64_t p = rp[r]; p < rp[r + 1]; ++p) {
        const int64_t c = col[p];
        bool good = !(p > rp[r] && col[p - 1] >= c);
        if (good && c == r) {
          good = vals[p].imag() == 0.0;
        } else if (good && c > r) {
          if (c < n) ++up;
        } else if (good) {
          ++lo;
          const int32_t* b = col.data() + rp[c];
          const int32_t* e = col.data() + rp[c + 1];
          const int32_t* q = std::lower_bound(b, e, (int32_t)r);
          good = q != e && *q == (int32_t)r;
          if (good) {
            const cplx t = vals[(size_t)(q - col.data())];
            good = t.real() == vals[p].real() && t.imag() == -vals[p].imag();
          }
        }
        if (!good) {
          ok.store(false, std::memory_order_relaxed);
          return;
        }
      }
    }
    nlower.fetch_add(lo, std::memory_order_relaxed);
    nupper.fetch_add(up, std::memory_order_relaxed);
  });
  return ok.load() && nlower.load() == nupper.load();
}

bool planes_all_real(const Planes& planes) {
  std::atomic<bool> all_real{true};
  for (const auto& pv : planes)
    parallel_rows((int64_t)pv.size(), [&](int64_t i0, int64_t i1) {
      for (int64_t i = i0; i < i1 && all_real.load(std::memory_order_relaxed); ++i)
        if (pv[(size_t)i].imag() != 0.0) all_real.store(false, std::memory_order_relaxed);
    }, (int64_t)1 << 20);
  return all_real.load();
}

void csr_value_map(const HostLayout& L, int64_t nrows, const UnionRowptr& ur, const UnionCols& uc, std::vector<int64_t>& map) {
  map.assign((size_t)std::max<int64_t>(ur[nrows], 1), 0);
  parallel_rows(nrows, [&](int64_t r_begin, int64_t r_end) {
    for (int64_t r = r_begin; r < r_end; ++r)
      for (int64_t k = 0; k < ur[r + 1] - ur[r]; ++k) map[ur[r] + k] = value_position(L, ur, uc, r, k);
  });
}

void plane_device_order(const HostLayout& L, const UnionRowptr& ur, const UnionCols& uc, const PlaneView& pv, int64_t r0, int64_t r1,
                        int64_t p0, int64_t p1, cplx* dst, int64_t fill_serial_below, int64_t scatter_serial_below) {
  parallel_rows(p1 - p0, [&](int64_t a, int64_t b) { std::fill(dst + a, dst + b, cplx(0.0)); }, fill_serial_below);
  parallel_rows(r1 - r0, [&](int64_t a, int64_t b) {
    for (int64_t r = r0 + a; r < r0 + b; ++r) {
      const int64_t nl = (L.format == QP_FMT_HRB) ? L.nlow[r] : 0;      // (the lower entries are not stored)
      for (int64_t k = nl; k < ur[r + 1] - ur[r]; ++k) dst[value_position(L, ur, uc, r, k) - p0] = pv[ur[r] + k];
    }
  }, scatter_serial_below);
}

// ---- row-block pointers ----------------------------------------------------------------------------------------------
void block_pointers(int64_t nrows, const UnionRowptr& ur, const UnionCols& uc, HostLayout& L) {
  const bool hrb = (L.format == QP_FMT_HRB);
  const int64_t nblocks = (nrows + kRB - 1) / kRB;
  L.bptr.assign(nblocks + 1, 0);
  if (hrb) {
    L.lptr.assign(nblocks + 1, 0);
    L.nlow.assign(nrows, 0);
    parallel_rows(nrows, [&](int64_t r0, int64_t r1) {
      for (int64_t r = r0; r < r1; ++r) {
        const int32_t* b = uc.data() + ur[r];
        L.nlow[r] = (int32_t)(std::lower_bound(b, uc.data() + ur[r + 1], (int32_t)r) - b);
      }
    });
  }
  // widths per block on a few threads (into the pointer arrays), then the running sums
  parallel_rows(nblocks, [&](int64_t b0, int64_t b1) {
    for (int64_t b = b0; b < b1; ++b) {
      int64_t wu = 0, wl = 0;
      for (int64_t r = b * kRB; r < std::min(nrows, (b + 1) * kRB); ++r) {
        const int64_t len = ur[r + 1] - ur[r];
        const int64_t nl = hrb ? L.nlow[r] : 0;
        wu = std::max(wu, len - nl);
        wl = std::max(wl, nl);
      }
      L.bptr[b + 1] = ((wu + 3) & ~(int64_t)3) * kRB;
      if (hrb) L.lptr[b + 1] = ((wl + 3) & ~(int64_t)3) * kRB;
    }
  }, 1024);
  for (int64_t b = 0; b < nblocks; ++b) {
    L.bptr[b + 1] += L.bptr[b];
    if (hrb) L.lptr[b + 1] += L.lptr[b];
  }
  L.stored = L.bptr[nblocks] + kRB;   // + one block of slack: padded lower entries read vals[0..63]
  L.lstored = hrb ? L.lptr[nblocks] : 0;
}

// ---- column sections -------------------------------------------------------------------------------------------------
constexpr size_t kBlockMapQuad = 16 + 4 * (size_t)kRB;   // bytes per quad of a block-map section: four column blocks + four lane bytes per row

// Encode the quad-packed column sections of blocks [b0, b1) into `bytes`, which starts empty (the offsets in meta[b] are
// relative to it): per block either int32 columns or, if every entry is within +-32767 of its row, int16 deltas to the row
// (2 bytes of index traffic per entry instead of 4).  `get(r, k, &is_pad)` returns the column of entry k of row r in this
// section (pad entries: any valid column).  `special(b, w, out)`: a chance to emit a block in the stencil encoding (returns
// true and appends its bytes) before the per-entry encodings are tried.
template <class GetCol, class Special>
static void encode_col_sections_range(int64_t nrows, int64_t ncols, int64_t b0, int64_t b1, const std::vector<int64_t>& ptr, GetCol& get,
                                      Special& special, std::vector<char>& bytes, std::vector<int64_t>& meta, bool allow_block_map) {
  // (pad entries multiply a zero value with x[column]: the column must exist.  A TALL operator -- fewer columns than rows --
  // has rows beyond its last column: a pad takes min(row, ncols - 1), never the row itself.)
  const int64_t last_col = std::max<int64_t>(ncols - 1, 0);
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t w = (ptr[b + 1] - ptr[b]) / kRB;
    while (bytes.size() % 32) bytes.push_back(0);
    const size_t start = bytes.size();
    if (w > 0 && special(b, w, bytes)) {
      meta[b] = ((int64_t)start << 2) | qp::kColStencil;
      continue;
    }
    // Block map: every slot sends the 64 rows of the block into ONE 64-aligned block of columns (any lane to any lane of it)
    // -- the structure of qubit-register Hamiltonians, where a Pauli string couples row and row XOR mask: 64-row blocks map
    // onto 64-row blocks, but the distance is +2^i or -2^i by the row's own bit, so no block-wide distance exists.  Per quad of
    // slots: four column-block numbers for the whole block (a wave-uniform load) + one byte per row and slot (the lane inside
    // the column block): 1.06 bytes of index traffic per entry instead of 4 (transverse-field Ising chain of 20 spins:
    // 101 -> 27 MB of index bytes per term).
    if (allow_block_map && w > 0 && (w % 4) == 0) {
      std::vector<int64_t> cb((size_t)w, -1);
      bool okmap = true;
      for (int64_t l = 0; l < kRB && okmap; ++l) {
        const int64_t r = b * kRB + l;
        if (r >= nrows) break;
        for (int64_t k = 0; k < w; ++k) {
          bool pad = false;
          const int64_t c = get(r, k, &pad);
          if (pad) continue;
          if (cb[(size_t)k] < 0) cb[(size_t)k] = c >> 6;
          else if (cb[(size_t)k] != (c >> 6)) { okmap = false; break; }
        }
      }
      if (okmap) {
        const int64_t own = std::min(std::min(b, (nrows - 1) >> 6), last_col >> 6);
        for (int64_t k = 0; k < w; ++k)
          if (cb[(size_t)k] < 0) cb[(size_t)k] = own;          // a slot of pure padding: any valid column will do
        meta[b] = ((int64_t)bytes.size() << 2) | qp::kColBlockMap;
        const size_t off = bytes.size();
        bytes.resize(off + (size_t)(w / 4) * kBlockMapQuad, 0);
        for (int64_t k = 0; k < w; ++k) {
          const int32_t c32 = (int32_t)cb[(size_t)k];
          std::memcpy(&bytes[off + (size_t)(k >> 2) * kBlockMapQuad + (size_t)(k & 3) * 4], &c32, 4);
        }
        for (int64_t l = 0; l < kRB; ++l) {
          const int64_t r = b * kRB + l;
          for (int64_t k = 0; k < w; ++k) {
            bool pad = (r >= nrows);
            const int64_t c = pad ? 0 : get(r, k, &pad);
            // pad entries (value 0) and the lanes beyond the last row: lane 0 of the slot's column block (a real column: the
            // block holds a real entry of this slot, or it is the row block itself)
            bytes[off + (size_t)(k >> 2) * kBlockMapQuad + 16 + (size_t)l * 4 + (size_t)(k & 3)] = pad ? (char)0 : (char)(c & 63);
          }
        }
        continue;
      }
    }
    bool ok16 = true;
    for (int64_t l = 0; l < kRB && ok16; ++l) {
      const int64_t r = b * kRB + l;
      if (r >= nrows) break;
      for (int64_t k = 0; k < w; ++k) {
        bool pad = false;
        const int64_t c = get(r, k, &pad);
        if (!pad && (c - r > 32767 || r - c > 32767)) { ok16 = false; break; }
      }
      if (r - std::min(r, last_col) > 32767) ok16 = false;   // (a pad of this row could not be encoded as a distance)
    }
    meta[b] = ((int64_t)bytes.size() << 2) | (ok16 ? qp::kColInt16 : qp::kColInt32);
    const size_t esz = ok16 ? 2 : 4;
    const size_t off = bytes.size();
    bytes.resize(off + (size_t)w * kRB * esz, 0);
    for (int64_t l = 0; l < kRB; ++l) {
      const int64_t r = b * kRB + l;
      const int64_t rc = std::min(r, nrows - 1);   // the kernel decodes deltas against the clamped row
      for (int64_t k = 0; k < w; ++k) {
        bool pad = (r >= nrows);
        int64_t c = pad ? std::min(rc, last_col) : get(r, k, &pad);
        if (pad && ok16) c = std::min(rc, last_col);
        const size_t q = (size_t)(k >> 2) * (4 * kRB) + (size_t)l * 4 + (k & 3);   // quad-packed slot
        if (ok16) {
          const int16_t d = (int16_t)(c - rc);
          std::memcpy(&bytes[off + q * 2], &d, 2);
        } else {
          const int32_t c32 = (int32_t)c;
          std::memcpy(&bytes[off + q * 4], &c32, 4);
        }
      }
    }
  }
  while (bytes.size() % 32) bytes.push_back(0);
}

// All blocks, in chunks on a few host threads (every block's bytes depend on that block alone; a block starts on a 32-byte boundary,
// so the chunks concatenate -- each padded to that boundary -- into exactly the bytes a single pass writes).
template <class GetCol, class Special>
static void encode_col_sections(int64_t nrows, int64_t ncols, const std::vector<int64_t>& ptr, GetCol get, Special special,
                                std::vector<char>& bytes, std::vector<int64_t>& meta, bool allow_block_map) {
  const int64_t nblocks = (int64_t)ptr.size() - 1;
  meta.assign((size_t)nblocks, 0);
  bytes.clear();
  const unsigned T = (nblocks >= 4096) ? host_threads() : 1u;
  if (T <= 1) {
    encode_col_sections_range(nrows, ncols, 0, nblocks, ptr, get, special, bytes, meta, allow_block_map);
    return;
  }
  std::vector<std::vector<char>> part((size_t)T);
  const int64_t chunk = (nblocks + T - 1) / T;
  parallel_rows((int64_t)T, [&](int64_t t0, int64_t t1) {
    for (int64_t t = t0; t < t1; ++t) {
      const int64_t c0 = std::min(nblocks, t * chunk), c1 = std::min(nblocks, (t + 1) * chunk);
      encode_col_sections_range(nrows, ncols, c0, c1, ptr, get, special, part[(size_t)t], meta, allow_block_map);
    }
  }, 0);
  for (unsigned t = 0; t < T; ++t) {
    while (bytes.size() % 32) bytes.push_back(0);
    const int64_t base = (int64_t)bytes.size();
    const int64_t c0 = std::min<int64_t>(nblocks, (int64_t)t * chunk), c1 = std::min<int64_t>(nblocks, (int64_t)(t + 1) * chunk);
    for (int64_t bb = c0; bb < c1; ++bb) meta[(size_t)bb] += base << 2;
    bytes.insert(bytes.end(), part[(size_t)t].begin(), part[(size_t)t].end());
    std::vector<char>().swap(part[(size_t)t]);
  }
}

// Stencil blocks: every row of the 64-row block has its k-th entry at the same distance
// delta_k from the diagonal (grids, lattices, tensor-product operators: most blocks of a
// banded H).  The section then stores w int32 deltas for the whole block instead of w x 64
// per-lane indices: the index stream disappears from HBM traffic (wave-uniform loads).
// Pad entries (value 0) take the block's delta too, so row + delta must stay a valid column.
template <class GetCol>
static bool try_stencil_upper(int64_t nrows, int64_t ncols, int64_t b, int64_t w, GetCol get, std::vector<char>& out) {
  std::vector<int32_t> delta((size_t)w, 0);
  for (int64_t k = 0; k < w; ++k) {
    bool have = false;
    int64_t d = 0;
    for (int64_t l = 0; l < kRB; ++l) {
      const int64_t r = b * kRB + l;
      if (r >= nrows) break;
      bool pad = false;
      const int64_t c = get(r, k, &pad);
      if (pad) continue;
      if (!have) {
        d = c - r;
        have = true;
      } else if (c - r != d) {
        return false;
      }
    }
    if (!have) d = 0;   // a slot of pure padding (width rounded up to a quad): column = row
    if (d > INT32_MAX || d < INT32_MIN) return false;
    // every lane (pad entries and the clamped rows of a partial last block included) must
    // land on a valid column
    const int64_t r_lo = b * kRB, r_hi = std::min(b * kRB + kRB - 1, nrows - 1);
    if (r_lo + d < 0 || r_hi + d >= ncols) return false;
    delta[(size_t)k] = (int32_t)d;
  }
  const size_t off = out.size();
  out.resize(off + (size_t)w * 4);
  std::memcpy(&out[off], delta.data(), (size_t)w * 4);
  return true;
}

void encode_upper_sections(int64_t nrows, int64_t ncols, const UnionRowptr& ur, const UnionCols& uc, HostLayout& L, bool stencil,
                           bool block_map, std::vector<char>& bytes) {
  const bool hrb = (L.format == QP_FMT_HRB);
  auto get_upper = [&](int64_t r, int64_t k, bool* pad) -> int64_t {
    const int64_t nl = hrb ? L.nlow[r] : 0;
    const int64_t len = ur[r + 1] - ur[r] - nl;
    if (k < len) return uc[ur[r] + nl + k];
    *pad = true;
    return (ur[r + 1] > ur[r]) ? uc[ur[r]] : 0;
  };
  encode_col_sections(nrows, ncols, L.bptr, get_upper,
                      [&](int64_t b, int64_t w, std::vector<char>& out) { return stencil && try_stencil_upper(nrows, ncols, b, w, get_upper, out); },
                      bytes, L.cmeta, block_map);
}

void transposed_positions(int64_t nrows, const UnionRowptr& ur, const UnionCols& uc, const HostLayout& L, qp::HostVec<int32_t>& lpos) {
  lpos.resize((size_t)std::max<int64_t>(L.lstored, 1));      // (half a gigabyte at N = 2^24: filled on the host threads, not by one)
  parallel_rows((int64_t)lpos.size(), [&](int64_t a, int64_t b) { std::fill(lpos.begin() + a, lpos.begin() + b, (int32_t)-1); }, (int64_t)1 << 20);
  parallel_rows(nrows, [&](int64_t r_begin, int64_t r_end) {
    for (int64_t r = r_begin; r < r_end; ++r)
      for (int64_t k = 0; k < L.nlow[r]; ++k) lpos[rb_quad_pos(L.lptr, r, k)] = (int32_t)(-value_position(L, ur, uc, r, k) - 1);
  });
}

// stencil lower block: every row has a real entry in every slot, at a block-wide distance delta_k, and the conj-transposed
// values sit at one slot per column block (at most two column blocks per slot): position = pb(column block) + column % 64
static bool try_stencil_lower(int64_t nrows, const UnionRowptr& ur, const UnionCols& uc, const HostLayout& L,
                              const qp::HostVec<int32_t>& lpos, int64_t b, int64_t w, std::vector<char>& out) {
  std::vector<LowerStencilSlot> slots((size_t)w);
  for (int64_t k = 0; k < w; ++k) {
    LowerStencilSlot e{0, 0, -1, -1, 0};
    bool have = false;
    for (int64_t l = 0; l < kRB; ++l) {
      const int64_t r = b * kRB + l;
      if (r >= nrows) break;
      if (k >= L.nlow[r]) return false;
      const int64_t c = uc[ur[r] + k];
      const int64_t base = (int64_t)lpos[rb_quad_pos(L.lptr, r, k)] - (c & 63);
      if (!have) {
        e.delta = (int32_t)(c - r);
        e.cb0 = (int32_t)(c >> 6);
        e.pb0 = base;
        have = true;
      } else if (c - r != e.delta) {
        return false;
      }
      if ((c >> 6) == e.cb0) {
        if (base != e.pb0) return false;
      } else if ((c >> 6) == e.cb0 + 1) {
        if (e.pb1 < 0) e.pb1 = base;
        else if (base != e.pb1) return false;
      } else {
        return false;
      }
    }
    if (!have) return false;
    if (e.pb1 < 0) e.pb1 = e.pb0;
    slots[(size_t)k] = e;
  }
  const size_t off = out.size();
  out.resize(off + (size_t)w * sizeof(LowerStencilSlot));
  std::memcpy(&out[off], slots.data(), (size_t)w * sizeof(LowerStencilSlot));
  return true;
}

void encode_lower_sections(int64_t nrows, int64_t ncols, const UnionRowptr& ur, const UnionCols& uc, HostLayout& L,
                           const qp::HostVec<int32_t>& lpos, bool stencil, bool block_map, std::vector<char>& bytes) {
  encode_col_sections(nrows, ncols, L.lptr,
                      [&](int64_t r, int64_t k, bool* pad) -> int64_t {
                        if (k < L.nlow[r]) return uc[ur[r] + k];
                        *pad = true;          // padded: any valid column, value masked by pos < 0
                        return r;
                      },
                      [&](int64_t b, int64_t w, std::vector<char>& out) { return stencil && try_stencil_lower(nrows, ur, uc, L, lpos, b, w, out); },
                      bytes, L.lcmeta, block_map);
}

int64_t decode_col(const std::vector<char>& bytes, const std::vector<int64_t>& meta, int64_t nrows, int64_t r, int64_t k, bool lower) {
  const int64_t m = meta[r / kRB];
  const size_t off = (size_t)(m >> 2);
  const int mode = (int)(m & 3);
  if (mode == qp::kColStencil) {
    int32_t d;
    std::memcpy(&d, &bytes[off + (size_t)k * (lower ? sizeof(LowerStencilSlot) : 4)], 4);
    return std::min(r, nrows - 1) + d;
  }
  if (mode == qp::kColBlockMap) {
    int32_t cb;
    std::memcpy(&cb, &bytes[off + (size_t)(k >> 2) * kBlockMapQuad + (size_t)(k & 3) * 4], 4);
    const unsigned char ln = (unsigned char)bytes[off + (size_t)(k >> 2) * kBlockMapQuad + 16 + (size_t)(r % kRB) * 4 + (size_t)(k & 3)];
    return ((int64_t)cb << 6) | (int64_t)ln;
  }
  const size_t q = (size_t)(k >> 2) * (4 * kRB) + (size_t)(r % kRB) * 4 + (k & 3);
  if (mode == qp::kColInt16) {
    int16_t d;
    std::memcpy(&d, &bytes[off + q * 2], 2);
    return std::min(r, nrows - 1) + d;
  }
  int32_t c;
  std::memcpy(&c, &bytes[off + q * 4], 4);
  return c;
}

int64_t decode_lower_stencil_pos(const std::vector<char>& bytes, const std::vector<int64_t>& meta, int64_t nrows, int64_t r, int64_t k) {
  const int64_t m = meta[r / kRB];
  LowerStencilSlot e;
  std::memcpy(&e, &bytes[(size_t)(m >> 2) + (size_t)k * sizeof(LowerStencilSlot)], sizeof(e));
  const int64_t c = std::min(r, nrows - 1) + e.delta;
  return ((c >> 6) == e.cb0 ? e.pb0 : e.pb1) + (c & 63);
}

// ---- sparse control terms (qp_operator::sparse_from) ---------------------------------------------------------------------
SparseControls find_sparse_controls(const HostLayout& L, int64_t nrows, int64_t stored, const UnionRowptr& ur, const UnionCols& uc,
                                    const Planes& planes, int ncoeffs, int max_terms) {
  SparseControls out;
  const int nops = (int)planes.size();
  const size_t limit = (size_t)(stored / 4);
  // per term, from the last one down while they stay sparse: the stored positions it touches, with its values there
  std::vector<std::vector<std::pair<int32_t, cplx>>> touched;
  int sfrom = nops;
  while (sparse_candidate(nops, ncoeffs, stored, sfrom - 1)) {
    const PlaneView& pv = planes[(size_t)(sfrom - 1)];
    std::vector<std::pair<int32_t, cplx>> t;
    for (int64_t r = 0; r < nrows && t.size() <= limit; ++r) {
      const int64_t nl = (L.format == QP_FMT_HRB) ? L.nlow[r] : 0;
      for (int64_t k = nl; k < ur[r + 1] - ur[r] && t.size() <= limit; ++k)
        if (pv[ur[r] + k] != cplx(0.0)) t.emplace_back((int32_t)value_position(L, ur, uc, r, k), pv[ur[r] + k]);
    }
    if (t.size() > limit) break;
    touched.push_back(std::move(t));
    --sfrom;
  }
  const size_t nsp = touched.size();
  if (nsp < 1 || nsp > (size_t)max_terms) return out;
  std::vector<int32_t>& sup = out.support;
  for (const auto& t : touched)
    for (const auto& e : t) sup.push_back(e.first);
  std::sort(sup.begin(), sup.end());
  sup.erase(std::unique(sup.begin(), sup.end()), sup.end());
  if (sup.empty() || (int64_t)sup.size() > stored / 4) return sup.clear(), out;
  out.support_vals.assign(nsp * sup.size(), cplx(0.0));
  for (size_t i = 0; i < nsp; ++i)      // touched[i] belongs to term nops - 1 - i
    for (const auto& e : touched[i])
      out.support_vals[(nsp - 1 - i) * sup.size() + (size_t)(std::lower_bound(sup.begin(), sup.end(), e.first) - sup.begin())] = e.second;
  out.sparse_from = sfrom;
  return out;
}

// ---- value dictionary ------------------------------------------------------------------------------------------------
// Per 64-row block the distinct tuples (value in term 0, .., value in term L - 1) over its stored positions (pads: the all-zero
// tuple), sorted bytewise; one code byte per stored position; tables with the same content shared.  Built when every block has at
// most 256 tuples and codes + tables come to less than half of the value plane the mat-vec would stream instead.
void build_value_dict(bool knob_on, int64_t nrows, int64_t nblocks, int64_t stored, bool planes_real, const HostLayout& Lh,
                      const UnionRowptr& ur, const Planes& planes, ValueDict& out) {
  out = ValueDict();
  if (!knob_on) return void(out.reason = 4);
  if (Lh.format != QP_FMT_RBCSR || stored <= 0 || nblocks <= 0) return void(out.reason = 1);
  const int L = (int)planes.size();
  const size_t tb = sizeof(cplx) * (size_t)L;       // bytes of one tuple
  std::vector<uint8_t> codes((size_t)stored, 0);
  std::vector<std::string> tables((size_t)nblocks);  // block b's sorted distinct tuples, tb bytes each
  std::atomic<bool> too_many{false};
  parallel_rows(nblocks, [&](int64_t b0, int64_t b1) {
    std::vector<char> ent;          // the block's tuples, position-major (slot, lane)
    std::vector<int32_t> order, code_of;
    for (int64_t b = b0; b < b1 && !too_many.load(std::memory_order_relaxed); ++b) {
      const int64_t w = (Lh.bptr[b + 1] - Lh.bptr[b]) / kRB;
      const int64_t npos = w * kRB;
      ent.assign((size_t)npos * tb, 0);
      for (int64_t l = 0; l < kRB; ++l) {
        const int64_t r = b * kRB + l;
        if (r >= nrows) break;
        const int64_t len = ur[r + 1] - ur[r];
        for (int64_t k = 0; k < len; ++k)
          for (int t = 0; t < L; ++t)
            std::memcpy(&ent[(size_t)(k * kRB + l) * tb + (size_t)t * sizeof(cplx)], &planes[(size_t)t][(size_t)(ur[r] + k)], sizeof(cplx));
      }
      // distinct tuples: sort the positions by tuple bytes, walk the runs
      order.resize((size_t)npos);
      for (int64_t i = 0; i < npos; ++i) order[(size_t)i] = (int32_t)i;
      std::sort(order.begin(), order.end(), [&](int32_t a, int32_t c) {
        return std::memcmp(&ent[(size_t)a * tb], &ent[(size_t)c * tb], tb) < 0;
      });
      code_of.assign((size_t)npos, 0);
      std::string& T = tables[(size_t)b];
      T.clear();
      int n = 0;
      bool fits = true;
      for (int64_t i = 0; i < npos; ++i) {
        const int32_t p = order[(size_t)i];
        if (i == 0 || std::memcmp(&ent[(size_t)p * tb], &ent[(size_t)order[(size_t)i - 1] * tb], tb) != 0) {
          if (n == 256) {
            fits = false;
            break;
          }
          T.append(&ent[(size_t)p * tb], tb);
          ++n;
        }
        code_of[(size_t)p] = n - 1;
      }
      if (!fits) {
        too_many.store(true, std::memory_order_relaxed);
        break;
      }
      // codes in the quad-packed layout of the column sections: byte (k & 3) of dword (k >> 2) * 64 + lane
      for (int64_t k = 0; k < w; ++k)
        for (int64_t l = 0; l < kRB; ++l) codes[(size_t)rb_quad_pos(Lh.bptr, b * kRB + l, k)] = (uint8_t)code_of[(size_t)(k * kRB + l)];
    }
  }, 64);
  if (too_many.load()) return void(out.reason = 2);
  // shared tables: first block with a content owns it
  std::unordered_map<std::string, int64_t> where;
  std::vector<int64_t> tptr((size_t)nblocks);
  std::string all;
  for (int64_t b = 0; b < nblocks; ++b) {
    auto it = where.find(tables[(size_t)b]);
    if (it == where.end()) {
      it = where.emplace(tables[(size_t)b], (int64_t)(all.size() / tb)).first;
      all += tables[(size_t)b];
    }
    tptr[(size_t)b] = (it->second << 9) | (int64_t)(tables[(size_t)b].size() / tb);   // first entry << 9 | entries (<= 256)
    std::string().swap(tables[(size_t)b]);
  }
  const int64_t ntab = (int64_t)(all.size() / tb);
  // what a term streams: a byte per stored position + (a share of) the tables, against 16 (8: real) bytes per position
  const double coded_bytes = (double)stored + 16.0 * (double)ntab, plain_bytes = (planes_real ? 8.0 : 16.0) * (double)stored;
  if (coded_bytes > 0.5 * plain_bytes) return void(out.reason = 3);
  out.ntab = ntab;
  out.ntables = (int64_t)where.size();
  out.codes.swap(codes);
  out.tptr.swap(tptr);
  out.tab.assign((size_t)L, std::vector<cplx>((size_t)ntab));
  for (int t = 0; t < L; ++t)
    for (int64_t e = 0; e < ntab; ++e) std::memcpy(&out.tab[(size_t)t][(size_t)e], &all[(size_t)e * tb + (size_t)t * sizeof(cplx)], sizeof(cplx));
}

void decode_value_dict(const HostLayout& L, int64_t nblocks, const std::vector<uint8_t>& codes, const std::vector<int64_t>& tptr,
                       const std::vector<cplx>& tab, std::vector<cplx>& hv) {
  for (int64_t b = 0; b < nblocks; ++b) {
    const int64_t w = (L.bptr[b + 1] - L.bptr[b]) / kRB;
    for (int64_t k = 0; k < w; ++k)
      for (int64_t r = b * kRB; r < (b + 1) * kRB; ++r)
        hv[(size_t)rb_val_pos(L.bptr, r, k)] = tab[(size_t)((tptr[(size_t)b] >> 9) + codes[(size_t)rb_quad_pos(L.bptr, r, k)])];
  }
}
