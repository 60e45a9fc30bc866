"""The Criteo ETL's contract as a plain Python / numpy loop: the reference's `getCriteoAdData`
(data_utils.py:876-1121: process_one_file, the dictionaries, processCriteoAdData, concatCriteoAdData) restated under the
stricter line grammar, with the two departures -- X_cat is int32, and a hash >= 2^31 keeps its bit pattern (ffffffff is -1).
It imports nothing from the package: tests/golden/criteo_etl.npz holds what the reference wrote for the same text and this
file must equal it bit for bit; it is then the yardstick for what the reference cannot produce (the wrap, the malformed-line
codes)."""
import numpy as np

N_DENSE, N_CAT = 13, 26
N_FIELDS = 1 + N_DENSE + N_CAT
ERR_FIELDS, ERR_DEC_BYTE, ERR_DEC_RANGE, ERR_HEX_BYTE, ERR_HEX_LONG, ERR_NOT_IN_DICT = 1, 2, 3, 4, 5, 6
_DEC = frozenset(b"0123456789")
_HEX = frozenset(b"0123456789abcdefABCDEF")


class Malformed(ValueError):
    def __init__(self, line1, code):
        ValueError.__init__(self, "line %d: code %d" % (line1, code))
        self.line1, self.code = line1, code


def split_lines(raw: bytes):
    """The lines of a file without their newline; a final line without one counts."""
    lines = raw.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def line_starts(chunk: bytes):
    """(starts, count) of the line-index rule: starts[0] = 0, starts[j + 1] one past the j-th newline."""
    starts = [0] + [p + 1 for p, c in enumerate(chunk) if c == 10]
    return np.array(starts, dtype=np.int64), len(starts) - 1


def parse_line(line: bytes, max_ind_range: int = -1):
    """(code, y, x_int [13], x_cat [26]); a malformed line gives its code and zeros."""
    fields = line.split(b"\t")
    code = 0
    vals = [0] * N_FIELDS
    for f, text in enumerate(fields[:N_FIELDS]):
        ferr, v = 0, 0
        if f <= N_DENSE:
            body = text[1:] if text[:1] == b"-" else text
            if any(c not in _DEC for c in body) or (text[:1] == b"-" and not body):
                ferr = ERR_DEC_BYTE
            else:
                v = int(text) if text else 0
                if not -2 ** 31 <= v <= 2 ** 31 - 1:
                    ferr = ERR_DEC_RANGE
                elif f >= 1 and v < 0:
                    v = 0
        else:
            if any(c not in _HEX for c in text):
                ferr = ERR_HEX_BYTE
            elif len(text) > 8:
                ferr = ERR_HEX_LONG
            else:
                v = int(text, 16) if text else 0
                if max_ind_range > 0:
                    v %= max_ind_range
                if v >= 2 ** 31:
                    v -= 2 ** 32
        vals[f] = 0 if ferr else v
        if ferr and not code:
            code = ferr
    if len(fields) != N_FIELDS:
        code = ERR_FIELDS
    if code:
        vals = [0] * N_FIELDS
    return code, vals[0], vals[1:1 + N_DENSE], vals[1 + N_DENSE:]


def parse_lines(lines, max_ind_range=-1):
    """(y [n], X_int [n, 13], X_cat [n, 26], errors): errors the (1-based line, code) of every malformed line, in order."""
    n = len(lines)
    y, x_int, x_cat = np.zeros(n, np.int32), np.zeros((n, N_DENSE), np.int32), np.zeros((n, N_CAT), np.int32)
    errors = []
    for k, line in enumerate(lines):
        code, y[k], x_int[k], x_cat[k] = parse_line(line, max_ind_range)
        if code:
            errors.append((k + 1, code))
    return y, x_int, x_cat, errors


def keep_mask(y, rand_u, rate):
    """data_utils.py:991-993: dropped iff the target is 0 and the line's draw is below the rate (float64)."""
    return ~((np.asarray(y) == 0) & (np.asarray(rand_u, dtype=np.float64) < np.float64(rate)))


def kaggle_split(total, days):
    """data_utils.py:926-929"""
    per, extras = divmod(total, days)
    return [per + (1 if j < extras else 0) for j in range(days)]


def etl(day_texts, max_ind_range=-1, sub_sample_rate=0.0, rng=np.random):
    """day_texts: the lines of every day file, in day order.  Returns dict(total_per_file, unique [26 arrays], counts,
    days = [(X_cat, X_int, y) per day], X_cat, X_int, y) -- every array as the ETL writes it.  Raises Malformed at the first
    bad line of a day file."""
    dicts = [{} for _ in range(N_CAT)]
    parsed, total_per_file = [], []
    for lines in day_texts:
        y, x_int, x_cat, errors = parse_lines(lines, max_ind_range)
        if errors:
            raise Malformed(*errors[0])
        if sub_sample_rate > 0.0:
            keep = keep_mask(y, rng.uniform(low=0.0, high=1.0, size=len(lines)), sub_sample_rate)
            y, x_int, x_cat = y[keep], x_int[keep], x_cat[keep]
        for row in x_cat:                                   # ids by first appearance, kept rows, day order
            for j in range(N_CAT):
                dicts[j].setdefault(int(row[j]), len(dicts[j]))
        parsed.append((y, x_int, x_cat))
        total_per_file.append(len(y))
    days = []
    for y, x_int, x_cat in parsed:
        enc = np.zeros_like(x_cat)
        for j in range(N_CAT):
            enc[:, j] = [dicts[j][int(v)] for v in x_cat[:, j]]
        days.append((enc, x_int, y))
    return dict(total_per_file=np.array(total_per_file, dtype=np.int64),
                unique=[np.array(list(d), dtype=np.int32) for d in dicts],
                counts=np.array([len(d) for d in dicts], dtype=np.int32), days=days,
                X_cat=np.concatenate([d[0] for d in days]), X_int=np.concatenate([d[1] for d in days]),
                y=np.concatenate([d[2] for d in days]))


def kaggle_days(raw: bytes, days=7):
    lines = split_lines(raw)
    out, at = [], 0
    for n in kaggle_split(len(lines), days):
        out.append(lines[at:at + n])
        at += n
    return out
