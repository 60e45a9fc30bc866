#!/usr/bin/env python3
"""Generate tests/golden/criteo_processed.npz by IMPORTING the reference, as tools/make_golden_bin.py does (same container,
same rules: only data travels -- the inputs and the reference's outputs for them).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_processed.py

A small synthetic processed file (X_int [230, 13], X_cat [230, 26], y, counts) and its day-count file, seven days of unequal
length -- one of exactly one row, one of exactly B = 16 rows, an odd last day (53 rows: test gets 27, val 26), 177 training rows
= 11 batches and a short one of a single row -- go through the reference's in-memory dataset path as `main` drives it
(main_no_ddp.py:509, :525 -> dlrm_data_pytorch.py:493-545): `np.random.seed(SEED)`, `CriteoDataset("train")`, then
`CriteoDataset("test")`, both batched by `DataLoader(..., collate_fn=collate_wrapper_criteo)`, for --data-randomize total,
day and none, with --max-ind-range off (-1) and on (50).  Recorded per mode: every batch's (X, lS_i, T), the batch sizes, the
last batch's lS_o, and the next `np.random.randint` draw after the two constructions (what the generator is left at).
Categorical values lie inside their tables (the file can be trained on); a few tables are smaller than the range."""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

SEED = 4321
SIZES = [41, 1, 37, 16, 52, 30, 53]
B = 16
MIRS = (-1, 50)
COUNTS = [200, 7, 40, 100000, 12, 2 ** 31 - 1, 13, 250, 4, 9, 50, 51, 49, 2, 77, 10, 3, 16, 8, 123, 4000, 3, 6, 23, 5, 10]


def main():
    torch.set_num_threads(1)
    sys.dont_write_bytecode = True
    sys.path.insert(0, MG.REF)
    import dlrm_data_pytorch as DP
    from torch.utils.data import DataLoader
    rng = np.random.RandomState(53)
    n = sum(SIZES)
    # (the host test compares X bit for bit, and the last bit of torch.log(7.0) differs between processors -- 0x3ff91395, the
    # correctly rounded value, on some, 0x3ff91396 on others: the dense value 6 stays out of the file)
    x_int = np.array([v for v in range(20) if v != 6], dtype=np.int32)[rng.randint(0, 19, size=(n, 13))]
    edge = np.array([0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1], dtype=np.int64).astype(np.int32)
    where = rng.rand(n, 13) < 0.05
    x_int[where] = edge[rng.randint(0, len(edge), size=int(where.sum()))]
    x_cat = np.stack([rng.randint(0, c, size=n, dtype=np.int64) for c in COUNTS], axis=1).astype(np.int32)
    x_cat[rng.randint(0, n, size=6), 5] = 2 ** 31 - 2        # the widest table's last row
    y = rng.randint(0, 2, size=n).astype(np.int32)
    counts = np.array(COUNTS, dtype=np.int64)
    out = dict(sizes=np.array(SIZES), B=B, seed=SEED, max_ind_ranges=np.array(MIRS), X_int=x_int, X_cat=x_cat, y=y,
               counts=counts)
    with tempfile.TemporaryDirectory() as d:
        raw = os.path.join(d, "train.txt")
        pro = os.path.join(d, "kaggleAdDisplayChallenge_processed.npz")
        np.savez(pro, X_int=x_int, X_cat=x_cat, y=y, counts=counts)
        np.savez(os.path.join(d, "train_day_count.npz"), total_per_file=np.array(SIZES))

        def record(name, batches):
            out[name + "_sizes"] = np.array([b[3].shape[0] for b in batches])
            out[name + "_X"] = torch.cat([b[0] for b in batches])
            out[name + "_lS_i"] = torch.cat([b[2] for b in batches], dim=1)
            out[name + "_T"] = torch.cat([b[3] for b in batches])
            out[name + "_lS_o_last"] = batches[-1][1]
            assert all(torch.equal(b[1], torch.arange(b[3].shape[0]).repeat(26, 1)) for b in batches)

        for randomize in ("total", "day", "none"):
            for mir in MIRS:
                np.random.seed(SEED)
                sets = {}
                for split in ("train", "test"):
                    sets[split] = DP.CriteoDataset("kaggle", mir, 0.0, randomize, split, raw, pro, False)
                out["%s_next_draw" % randomize] = np.random.randint(0, 2 ** 31 - 1, size=4)
                for split, ds in sets.items():
                    ld = DataLoader(ds, batch_size=B, shuffle=False, num_workers=0, collate_fn=DP.collate_wrapper_criteo,
                                    pin_memory=False, drop_last=False)
                    name = "%s_%s_m%d" % (randomize, split, mir if mir > 0 else 0)
                    out[name + "_len"] = len(ld)
                    record(name, list(ld))
                assert sets["train"].m_den == 13 and sets["train"].n_emb == 26
    MG.save("criteo_processed", **out)


if __name__ == "__main__":
    main()
