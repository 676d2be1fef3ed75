// The one place where a device block passed as (rom_buf, offset, row stride, columns, rows) is checked on the host (internal,
// host only: no HIP call, compiles with a plain C++ compiler).  Nothing here multiplies or adds two caller-given sizes without
// looking at the carry: a block whose extent does not fit a size_t is a block that does not fit its buffer.
#pragma once
#include <cstddef>
#include <cstdint>

#include "romhc_internal.h"

// how the messages call the block, its stride and its column count: {"X", "ldx", "m"}
struct RomBlockNames {
  const char *block, *ld, *cols;
};

// doubles from the first entry to one past the last of `rows` rows of `cols` with stride ld: (rows - 1) ld + cols, or SIZE_MAX
// when there is no such row block (rows < 1, a negative size) or the extent wraps a size_t
inline size_t rom_block_span(int64_t rows, int64_t ld, int64_t cols) {
  size_t span = 0;
  if (rows < 1 || ld < 0 || cols < 0 || __builtin_mul_overflow(size_t(rows - 1), size_t(ld), &span) ||
      __builtin_add_overflow(span, size_t(cols), &span))
    return SIZE_MAX;
  return span;
}

// ld >= cols, and [off, off + span) inside the buf_doubles doubles of the buffer
inline int rom_check_block(const char* who, const RomBlockNames& nm, size_t buf_doubles, size_t off, int64_t ld, int cols, int64_t rows) {
  ROM_CHECK(ld >= cols, "%s: %s = %lld < %s = %d", who, nm.ld, (long long)ld, nm.cols, cols);
  const size_t span = rom_block_span(rows, ld, cols);
  ROM_CHECK(span <= buf_doubles && off <= buf_doubles - span,   // (a difference, not off + span: no carry)
            "%s: %s holds %zu doubles, %lld rows of %d at offset %zu with stride %lld need more", who, nm.block, buf_doubles,
            (long long)rows, cols, off, (long long)ld);
  return ROM_OK;
}

// two checked blocks, given by their first entries and spans, share a double
inline bool rom_blocks_overlap(const double* a, size_t span_a, const double* b, size_t span_b) { return a < b + span_b && b < a + span_a; }

// the row count of the map entry points: 1 .. 2^40
inline int rom_check_rows(const char* who, int64_t M) {
  ROM_CHECK(M >= 1 && M <= (int64_t(1) << 40), "%s: M = %lld rows, at least 1", who, (long long)M);
  return ROM_OK;
}

// The blocks of a map's *_predict: M rows of m inputs in X; OUT and Yref (either may be NULL) M rows of q, OUT apart from X
inline int rom_check_predict_blocks(const char* who, int64_t M, const rom_buf* X, size_t x_off, int64_t ldx, int m, int q, const rom_buf* OUT,
                                    size_t o_off, int64_t ldo, const rom_buf* Yref, size_t r_off, int64_t ldr) {
  ROM_TRY(rom_check_rows(who, M));
  ROM_TRY(rom_check_block(who, {"X", "ldx", "m"}, X->n, x_off, ldx, m, M));
  if (OUT) {
    ROM_TRY(rom_check_block(who, {"OUT", "ldo", "q"}, OUT->n, o_off, ldo, q, M));
    ROM_CHECK(!rom_blocks_overlap(X->p + x_off, rom_block_span(M, ldx, m), OUT->p + o_off, rom_block_span(M, ldo, q)),
              "%s: OUT overlaps X (the inputs are read while the predictions are written)", who);
  }
  if (Yref) ROM_TRY(rom_check_block(who, {"Yref", "ldr", "q"}, Yref->n, r_off, ldr, q, M));
  return ROM_OK;
}
