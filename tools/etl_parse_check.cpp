// The ETL's line parser on the CPU, under AddressSanitizer and UBSan, before it runs on a GPU:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cdlrm_amd/csrc
//         tools/etl_parse_check.cpp -o etl_parse_check;  ./etl_parse_check [raw-text-file ...]
//
// It includes csrc/etl_parse.h -- the SAME text csrc/etl.hip compiles for gfx950 -- and runs etl_parse_line over adversarial
// buffers and over every file named on the command line.  Each buffer is copied into a heap block of exactly its length, so a
// read one byte past a line's end is a read past the allocation, which the sanitizer reports.  The spans handed to the parser
// are the device's: the lines of the line index, and (what a wrong carry would hand over) the unfinished tail of the buffer.
// Prints one line per file, "<file>: lines N errors E sum S" (S: the sum of every output value), and exits 0 when every
// adversarial case gave the code it must.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "etl_parse.h"

struct Parsed {
    int code;
    int32_t y, x_int[ETL_N_DENSE], x_cat[ETL_N_CAT];
};

static int g_failures = 0;

static void expect(bool ok, const char* what, const std::string& name) {
    if (!ok) {
        fprintf(stderr, "FAIL %s: %s\n", name.c_str(), what);
        ++g_failures;
    }
}

// the buffer in a heap block of exactly its size; the codes of its lines, then (tail = true) of text[starts[n], len)
static std::vector<Parsed> run(const std::string& buf, int64_t max_ind_range, bool tail, int64_t* n_lines) {
    const int64_t len = (int64_t)buf.size();
    uint8_t* text = (uint8_t*)malloc((size_t)len);          // malloc(0): a block no byte of which may be read
    if (len) memcpy(text, buf.data(), (size_t)len);
    const int64_t n = etl_line_index_host(text, len, nullptr, 0);
    std::vector<int64_t> starts((size_t)n + 1);
    const int64_t n2 = etl_line_index_host(text, len, starts.data(), n);
    if (n2 != n) { fprintf(stderr, "FAIL line index not repeatable\n"); ++g_failures; }
    std::vector<Parsed> out;
    for (int64_t i = 0; i < n; ++i) {
        Parsed r;
        r.code = etl_parse_line(text, starts[i], starts[i + 1] - 1, max_ind_range, &r.y, r.x_int, r.x_cat);
        out.push_back(r);
    }
    if (tail) {
        Parsed r;
        r.code = etl_parse_line(text, starts[n], len, max_ind_range, &r.y, r.x_int, r.x_cat);
        out.push_back(r);
    }
    *n_lines = n;
    free(text);
    return out;
}

static bool all_zero(const Parsed& r) {
    if (r.y) return false;
    for (int k = 0; k < ETL_N_DENSE; ++k) if (r.x_int[k]) return false;
    for (int k = 0; k < ETL_N_CAT; ++k) if (r.x_cat[k]) return false;
    return true;
}

// a line of 40 fields: label, 13 dense, 26 hex; field f replaced by `with` when f >= 0
static std::string line(int f = -1, const std::string& with = "", int n_fields = ETL_N_FIELDS) {
    std::string s;
    for (int k = 0; k < n_fields; ++k) {
        if (k) s += '\t';
        if (k == f) s += with;
        else if (k == 0) s += "1";
        else if (k <= ETL_N_DENSE) s += std::to_string(k * 3 - 7);      // some negative
        else s += "a" + std::to_string(k) + "f";
    }
    return s;
}

static void one_code(const std::string& name, const std::string& buf, int want_code, int64_t want_lines = 1, bool tail = false) {
    int64_t n;
    std::vector<Parsed> r = run(buf, -1, tail, &n);
    expect(n == want_lines, "line count", name);
    if (r.empty()) { expect(want_code < 0, "no line parsed", name); return; }
    const Parsed& last = r.back();
    if (last.code != want_code) fprintf(stderr, "     got code %d, want %d\n", last.code, want_code);
    expect(last.code == want_code, "code", name);
    if (want_code) expect(all_zero(last), "a malformed line's outputs are zero", name);
}

int main(int argc, char** argv) {
    int64_t n;
    // ---- well-formed
    {
        std::vector<Parsed> r = run(line() + "\n", -1, false, &n);
        expect(n == 1 && r[0].code == ETL_OK && r[0].y == 1, "plain line", "plain");
        expect(r[0].x_int[0] == 0 && r[0].x_int[1] == 0 && r[0].x_int[2] == 2 && r[0].x_int[12] == 32, "dense clamp", "plain");
        expect(r[0].x_cat[0] == 0xa14f && r[0].x_cat[25] == 0xa39f, "hex", "plain");
        r = run(line(39, "") + "\n" + line(1, "") + "\n", -1, false, &n);
        expect(n == 2 && r[0].code == ETL_OK && r[0].x_cat[25] == 0 && r[1].code == ETL_OK && r[1].x_int[0] == 0, "empty fields", "empty");
        r = run(line(14, "7fffffff") + "\n" + line(14, "80000000") + "\n" + line(39, "FFFFffff") + "\n", -1, false, &n);
        expect(n == 3 && r[0].x_cat[0] == INT32_MAX && r[1].x_cat[0] == INT32_MIN && r[2].x_cat[25] == -1, "wrap", "wrap");
        r = run(line(14, "ffffffff") + "\n", 10, false, &n);
        expect(r[0].code == ETL_OK && r[0].x_cat[0] == 5 && r[0].x_cat[1] == (0xa15f % 10), "max_ind_range", "range");
        r = run(line(1, "-2147483648") + "\n" + line(1, "2147483647") + "\n" + line(0, "-2147483648") + "\n", -1, false, &n);
        expect(r[0].code == ETL_OK && r[0].x_int[0] == 0 && r[1].code == ETL_OK && r[1].x_int[0] == INT32_MAX &&
               r[2].code == ETL_OK && r[2].y == INT32_MIN, "int32 edges", "edges");
    }
    // ---- the adversarial buffers
    one_code("empty buffer", "", -1, 0);
    one_code("empty buffer, tail", "", ETL_ERR_FIELDS, 0, true);
    one_code("no trailing newline", line() + "\n" + line(), ETL_OK, 1);
    one_code("no trailing newline, tail", line() + "\n" + line(), ETL_OK, 1, true);
    {
        const std::string l = line();
        const size_t in_field = l.find('\t', 40) + 2, behind_tab = l.find('\t', 60) + 1;
        one_code("cut inside a field", line() + "\n" + l.substr(0, in_field), ETL_ERR_FIELDS, 1, true);
        one_code("cut right behind a tab", line() + "\n" + l.substr(0, behind_tab), ETL_ERR_FIELDS, 1, true);
        one_code("cut behind the last tab", l.substr(0, l.rfind('\t') + 1), ETL_OK, 0, true);      // an empty last field
    }
    one_code("39 fields", line(-1, "", 39) + "\n", ETL_ERR_FIELDS);
    one_code("41 fields", line(-1, "", 41) + "\n", ETL_ERR_FIELDS);
    one_code("400 fields", line(-1, "", 400) + "\n", ETL_ERR_FIELDS);
    one_code("lone -", line(3, "-") + "\n", ETL_ERR_DEC_BYTE);
    one_code("lone - as the label", line(0, "-") + "\n", ETL_ERR_DEC_BYTE);
    one_code("--1", line(3, "--1") + "\n", ETL_ERR_DEC_BYTE);
    one_code("+1", line(3, "+1") + "\n", ETL_ERR_DEC_BYTE);
    one_code("space", line(3, " 1") + "\n", ETL_ERR_DEC_BYTE);
    one_code("300 digits", line(5, std::string(300, '9')) + "\n", ETL_ERR_DEC_RANGE);
    one_code("300 digits, negative", line(5, "-" + std::string(300, '9')) + "\n", ETL_ERR_DEC_RANGE);
    one_code("300 zeros", line(5, std::string(300, '0')) + "\n", ETL_OK);
    one_code("2^31", line(5, "2147483648") + "\n", ETL_ERR_DEC_RANGE);
    one_code("-2^31 - 1", line(5, "-2147483649") + "\n", ETL_ERR_DEC_RANGE);
    one_code("300 hex digits", line(20, std::string(300, 'f')) + "\n", ETL_ERR_HEX_LONG);
    one_code("9 hex digits", line(20, "123456789") + "\n", ETL_ERR_HEX_LONG);
    one_code("9 hex digits, leading zero", line(39, "000000001") + "\n", ETL_ERR_HEX_LONG);
    one_code("hex g", line(20, "12g4") + "\n", ETL_ERR_HEX_BYTE);
    one_code("hex 0x", line(20, "0x12") + "\n", ETL_ERR_HEX_BYTE);
    one_code("hex -", line(20, "-1") + "\n", ETL_ERR_HEX_BYTE);
    one_code("bytes >= 0x80, decimal", line(2, "\x80\xff") + "\n", ETL_ERR_DEC_BYTE);
    one_code("bytes >= 0x80, hex", line(30, "\xc3\xa9") + "\n", ETL_ERR_HEX_BYTE);
    one_code("bytes >= 0x80 only", std::string(64, '\xff') + "\n", ETL_ERR_FIELDS);
    one_code("NUL", line(2, std::string(1, '\0')) + "\n", ETL_ERR_DEC_BYTE);
    one_code("\\r\\n", line() + "\r\n", ETL_ERR_HEX_BYTE);
    one_code("\\r\\n behind an empty field", line(39, "") + "\r\n", ETL_ERR_HEX_BYTE);
    one_code("only newlines", "\n\n\n\n\n", ETL_ERR_FIELDS, 5);
    one_code("only tabs", std::string(39, '\t') + "\n", ETL_OK);
    one_code("one byte", "7", ETL_ERR_FIELDS, 0, true);
    one_code("one newline", "\n", ETL_ERR_FIELDS, 1);
    // a bad byte wins inside a field, the field count over everything, the first field's error over a later one's
    one_code("bad byte and too long", line(20, "12345678g") + "\n", ETL_ERR_HEX_BYTE);
    one_code("first field's error", line(2, "x", 40).replace(0, 1, "2147483648") + "\n", ETL_ERR_DEC_RANGE);
    one_code("count over field", line(2, "x", 39) + "\n", ETL_ERR_FIELDS);

    // ---- files
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::string buf;
        char tmp[4096];
        size_t got;
        while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) buf.append(tmp, got);
        fclose(f);
        if (!buf.empty() && buf.back() != '\n') buf += '\n';             // a final line without '\n' counts as a line
        for (int64_t mir : {(int64_t)-1, (int64_t)10}) {
            std::vector<Parsed> r = run(buf, mir, false, &n);
            int64_t errors = 0, sum = 0;
            for (const Parsed& p : r) {
                errors += p.code != 0;
                sum += p.y;
                for (int k = 0; k < ETL_N_DENSE; ++k) sum += p.x_int[k];
                for (int k = 0; k < ETL_N_CAT; ++k) sum += p.x_cat[k];
            }
            printf("%s: range %lld lines %lld errors %lld sum %lld\n", argv[a], (long long)mir, (long long)n, (long long)errors,
                   (long long)sum);
        }
    }
    if (g_failures) {
        fprintf(stderr, "%d case(s) failed\n", g_failures);
        return 1;
    }
    printf("etl_parse_check: all cases ok\n");
    return 0;
}
