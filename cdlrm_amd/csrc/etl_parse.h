// One line of raw Criteo text -> (y, X_int[13], X_cat[26]).  The routine exists ONCE and compiles for the host and for
// gfx950: csrc/etl.hip runs it one lane per line, tools/etl_parse_check.cpp runs the same text of it on the CPU under
// AddressSanitizer / UBSan before it ever sees a GPU.  It restates the reference's per-line work (data_utils.py:984-1006,
// the clamp of :150) under the stricter grammar of DESIGN.md section 3; tests/etl_restated.py is the same contract in Python.
//
// The line is text[begin, end), WITHOUT its '\n'.  Nothing outside [begin, end) is read and every loop is bounded by end.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ETL_HD __host__ __device__
#else
#define ETL_HD
#endif

#define ETL_N_DENSE 13
#define ETL_N_CAT 26
#define ETL_N_FIELDS (1 + ETL_N_DENSE + ETL_N_CAT)

// codes of the device error word (low 8 bits; the 1-based line number of the file sits above them)
#define ETL_OK 0
#define ETL_ERR_FIELDS 1        // not exactly 40 tab-separated fields
#define ETL_ERR_DEC_BYTE 2      // a decimal field holds a byte outside [0-9] behind one optional leading '-' (a lone '-' too)
#define ETL_ERR_DEC_RANGE 3     // a decimal field outside int32
#define ETL_ERR_HEX_BYTE 4      // a hex field holds a byte outside [0-9a-fA-F]
#define ETL_ERR_HEX_LONG 5      // a hex field of more than 8 digits
#define ETL_ERR_NOT_IN_DICT 6   // cdlrm_etl_encode: a value its key array does not hold
#define ETL_ERR_SPAN 7          // cdlrm_etl_parse: a line span outside the text buffer (a line-index array that is not one)

// The first line with an error wins (smallest word); within a line a wrong field count wins over the first field's error;
// within a field a bad byte wins over range / length.  A malformed line's outputs are all zero.
ETL_HD static inline int etl_parse_line(const uint8_t* text, int64_t begin, int64_t end, int64_t max_ind_range, int32_t* y,
                                        int32_t* x_int, int32_t* x_cat) {
    int code = ETL_OK, field = 0;
    int64_t p = begin;
    for (;;) {                                            // one trip per field; p only grows and every trip ends at q <= end
        int64_t q = p;
        int ferr = ETL_OK;
        if (field <= ETL_N_DENSE) {                       // label and dense features: signed decimal int32, empty = 0
            bool neg = false, bad = false;
            int nd = 0;
            int64_t acc = 0;
            if (q < end && text[q] == '-') { neg = true; ++q; }
            for (; q < end && text[q] != '\t'; ++q) {
                const unsigned c = (unsigned)text[q] - (unsigned)'0';
                if (c > 9u) { bad = true; continue; }
                acc = acc * 10 + (int64_t)c;
                if (acc > 0x80000000ll) acc = 0x80000001ll;       // saturates: out of range whatever follows
                ++nd;
            }
            if (bad || (neg && nd == 0)) ferr = ETL_ERR_DEC_BYTE;
            else if (acc > (neg ? 0x80000000ll : 0x7fffffffll)) ferr = ETL_ERR_DEC_RANGE;
            const int32_t v = ferr ? 0 : (int32_t)(neg ? -acc : acc);
            if (field == 0) *y = v;
            else x_int[field - 1] = v < 0 ? 0 : v;        // X_int[X_int < 0] = 0
        } else if (field < ETL_N_FIELDS) {                // categorical hashes: hex, at most 8 digits, empty = 0
            bool bad = false;
            int nd = 0;
            uint32_t acc = 0;
            for (; q < end && text[q] != '\t'; ++q) {
                const unsigned c = text[q];
                unsigned d;
                if (c - (unsigned)'0' <= 9u) d = c - (unsigned)'0';
                else if ((c | 0x20u) - (unsigned)'a' <= 5u) d = (c | 0x20u) - (unsigned)'a' + 10u;
                else { bad = true; continue; }
                if (nd < 8) acc = (acc << 4) | d;
                if (nd < 9) ++nd;
            }
            if (bad) ferr = ETL_ERR_HEX_BYTE;
            else if (nd > 8) ferr = ETL_ERR_HEX_LONG;
            if (max_ind_range > 0) acc = (uint32_t)((int64_t)acc % max_ind_range);
            // a value >= 2^31 keeps its bit pattern: ffffffff is -1 (what numpy < 1.24 stored)
            int32_t v;
            if (ferr) v = 0;
            else if (acc & 0x80000000u) v = (int32_t)(acc & 0x7fffffffu) + INT32_MIN;
            else v = (int32_t)acc;
            x_cat[field - 1 - ETL_N_DENSE] = v;
        } else {                                          // fields past the 40th: only counted
            for (; q < end && text[q] != '\t'; ++q) {}
        }
        if (ferr && !code) code = ferr;
        if (q >= end) break;
        p = q + 1;                                        // text[q] is the tab
        if (field < ETL_N_FIELDS) ++field;                // (saturates: a line cannot overflow the counter)
    }
    if (field != ETL_N_FIELDS - 1) code = ETL_ERR_FIELDS;
    if (code) {
        *y = 0;
        for (int k = 0; k < ETL_N_DENSE; ++k) x_int[k] = 0;
        for (int k = 0; k < ETL_N_CAT; ++k) x_cat[k] = 0;
    }
    return code;
}

// The line-index rule on the host (what cdlrm_etl_line_index computes on the device): starts[0] = 0, starts[j + 1] = one
// past the j-th '\n'; returns the number of lines that END inside text[0, len) -- bytes behind the last '\n' are no line.
// starts may be null (count only); at most cap + 1 entries are written.
static inline int64_t etl_line_index_host(const uint8_t* text, int64_t len, int64_t* starts, int64_t cap) {
    int64_t n = 0;
    if (starts && cap >= 0) starts[0] = 0;
    for (int64_t p = 0; p < len; ++p)
        if (text[p] == '\n') {
            ++n;
            if (starts && n <= cap) starts[n] = p + 1;
        }
    return n;
}
