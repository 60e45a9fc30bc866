"""cdlrm_amd.main_no_ddp with a dump of every rank's cache tags after each window commit, for tests/test_insert_fill.py:
    python tests/insert_fill_cli_dump.py <prefix> <CLI flags ...>      (one rank, or under the launcher)
writes <prefix>.rank<r>: a list of the flat tag tensors, one per commit."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from cdlrm_amd import engine, main_no_ddp
    prefix, argv = sys.argv[1], sys.argv[2:]
    snaps = []
    real_commit = engine.WindowPipeline.commit

    def commit(self):
        real_commit(self)
        torch.cuda.synchronize()
        snaps.append(self.cg.tags.cpu().clone())

    engine.WindowPipeline.commit = commit
    main_no_ddp.main(argv)
    torch.save(snaps, "%s.rank%s" % (prefix, os.environ.get("RANK", "0")))


if __name__ == "__main__":
    main()
