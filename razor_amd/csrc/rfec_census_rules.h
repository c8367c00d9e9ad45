/* rfec_census_rules.h -- which plan a receiver takes for a SIM_FEC's (count, row, col), stated once as plain C:
 * rfec_plan_from_key (rfec_host.c) builds the plan, rfec_census.hip's kernels ask for the line a record's index
 * names in it, and both go through the two functions below, so the device and the host cannot disagree.  gcc and
 * hipcc compile it; not installed.
 *
 * The plan of a plannable key is rfec_plan_matrix(count, row, col, layers) with layers = ROWS | COLS for the
 * matrix key of its count -- count >= 6 and (row, col) what rfec_num_packets(count, 255) returns: the planner's
 * matrix mode -- and ROWS for any other key.  Its lines, in plan order (build_plan, rfec_host.c):
 *   row r, index r          members r col .. of which at least two lie below count: r < row and r col + 2 <= count.
 *                           The rows that have a line are a prefix of the rows, so row r is line r; with
 *                           count <= 128 and col >= 2 there are at most 64 of them (RFEC_MAX_LINES)
 *   column c, index 0x80|c  the matrix key alone, row > 1: members c, c + col, .. of which at least two lie below
 *                           count: c < col and c + col < count.  Those columns are a prefix too: column c is line
 *                           (rows with a line) + c
 * A row index is below 0x80 (at most 63), so no index names two lines. */
#ifndef RFEC_CENSUS_RULES_H_
#define RFEC_CENSUS_RULES_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define RFEC_CENSUS_FN static __host__ __device__ inline __attribute__((always_inline))
#else
#define RFEC_CENSUS_FN static inline
#endif

#define RFEC_CENSUS_NO_LINE 0xFFu
#define RFEC_CENSUS_MAX_COUNT 128u /* RFEC_MAX_K */

/* the plannable predicate: the keys rfec_plan_from_key has a plan for */
RFEC_CENSUS_FN int rfec_census_plannable(uint32_t count, uint32_t row, uint32_t col)
{
    return count >= 1 && count <= RFEC_CENSUS_MAX_COUNT && row >= 1 && col >= 2 && row * col >= count;
}

/* 1 when (count, row, col) is the matrix key of its count; (mrow, mcol): rfec_num_packets(count, 255) */
RFEC_CENSUS_FN int rfec_census_matrix_key(uint32_t count, uint32_t row, uint32_t col, uint32_t mrow, uint32_t mcol)
{
    return count >= 6 && row == mrow && col == mcol;
}

/* The line of the key's plan that a SIM_FEC's `index` names, or RFEC_CENSUS_NO_LINE: for an unplannable key, and for
 * an index that is no line of the plan.  (mrow, mcol): the matrix (row, col) of `count`, read only for count >= 6. */
RFEC_CENSUS_FN uint32_t rfec_census_line_of(uint32_t count, uint32_t row, uint32_t col, uint32_t index,
                                             uint32_t mrow, uint32_t mcol)
{
    if (!rfec_census_plannable(count, row, col))
        return RFEC_CENSUS_NO_LINE;
    if (index < 0x80u)
        return index < row && index * col + 2 <= count ? index : RFEC_CENSUS_NO_LINE;
    const uint32_t c = index & 0x7Fu;
    if (!rfec_census_matrix_key(count, row, col, mrow, mcol) || row < 2 || c >= col || c + col >= count)
        return RFEC_CENSUS_NO_LINE;
    const uint32_t last = (count - 2) / col; /* the last row with a line (count >= 6) */
    return (last + 1 < row ? last + 1 : row) + c;
}

#endif
