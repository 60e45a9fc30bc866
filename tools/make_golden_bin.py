#!/usr/bin/env python3
"""Generate tests/golden/criteo_bin.npz by IMPORTING the reference, as tools/make_golden.py does (same container, same rules:
only data travels -- inputs, the bytes of the files the reference wrote, and the reference's outputs for them).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_bin.py

Three tiny day arrays (23 / 14 / 17 rows, as criteo_loader.npz: 54 records, not a multiple of the batch size 7) are written
to binary files by the reference's own `numpy_to_binary` (train from the three days; `test` / `val` = the halves of the last
day) and read back through the reference's `CriteoBinDataset` + `torch.utils.data.DataLoader`, as
dlrm_data_pytorch.py:404-439 builds them: unshuffled for max_ind_range 50 and -1, and the training file with
`RandomSampler` for two epochs behind `torch.manual_seed(SEED)`.  A few categorical entries are negative: the modulus of the
reference (`%` on an int32 tensor) is the floor-mod."""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

SEED = 1234
SIZES = [23, 14, 17]
B = 7


def main():
    torch.set_num_threads(1)
    sys.dont_write_bytecode = True
    sys.path.insert(0, MG.REF)
    import data_loader_terabyte as DL
    from torch.utils.data import DataLoader, RandomSampler
    rng = np.random.RandomState(31)
    out = dict(sizes=np.array(SIZES), B=B, seed=SEED, max_ind_ranges=np.array([50, -1]))
    with tempfile.TemporaryDirectory() as d:
        days = []
        for day, n in enumerate(SIZES):
            xi = rng.randint(0, 1000, size=(n, 13)).astype(np.int32)
            xc = rng.randint(0, 100000, size=(n, 26)).astype(np.int32)
            neg = rng.rand(n, 26) < 0.1
            xc[neg] = -xc[neg] - 1
            y = rng.randint(0, 2, size=n).astype(np.int32)
            days.append(os.path.join(d, "day_%d_reordered.npz" % day))
            np.savez(days[-1], X_int=xi, X_cat=xc, y=y)
            out["xi_%d" % day], out["xc_%d" % day], out["y_%d" % day] = xi, xc, y
        counts = os.path.join(d, "day_fea_count.npz")
        np.savez(counts, counts=np.full(26, 100000))
        files = {}
        for split in ("train", "test", "val"):
            files[split] = os.path.join(d, split + ".bin")
            DL.numpy_to_binary(input_files=days if split == "train" else days[-1:], output_file_path=files[split], split=split)
            with open(files[split], "rb") as f:
                out[split + "_bytes"] = np.frombuffer(f.read(), dtype=np.uint8)

        def record(name, batches):
            out[name + "_sizes"] = np.array([b[3].shape[0] for b in batches])
            out[name + "_X"] = torch.cat([b[0] for b in batches])
            out[name + "_lS_i"] = torch.cat([b[2] for b in batches], dim=1)
            out[name + "_T"] = torch.cat([b[3] for b in batches])
            out[name + "_lS_o_last"] = batches[-1][1]

        for mir in (50, -1):
            for split in ("train", "test", "val"):
                ds = DL.CriteoBinDataset(data_file=files[split], counts_file=counts, batch_size=B, max_ind_range=mir)
                ld = DataLoader(ds, batch_size=None, batch_sampler=None, shuffle=False, num_workers=0, collate_fn=None,
                                pin_memory=False, drop_last=False)
                name = "%s_m%d" % (split, mir if mir > 0 else 0)
                out[name + "_len"] = len(ds)
                record(name, list(ld))

        seen = []

        class Recording(DL.CriteoBinDataset):       # the reference's class, telling which entries it is asked for
            def __getitem__(self, idx):
                seen.append(int(idx))
                return super().__getitem__(idx)

        ds = Recording(data_file=files["train"], counts_file=counts, batch_size=B, max_ind_range=50)
        torch.manual_seed(SEED)
        ld = DataLoader(ds, batch_size=None, batch_sampler=None, shuffle=False, num_workers=0, collate_fn=None,
                        pin_memory=False, drop_last=False, sampler=RandomSampler(ds))
        for epoch in range(2):
            del seen[:]
            record("shuffle_e%d" % epoch, list(ld))
            out["shuffle_e%d_order" % epoch] = np.array(seen)
    MG.save("criteo_bin", **out)


if __name__ == "__main__":
    main()
