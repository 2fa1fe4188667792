"""Child process of tests/test_gpu_box_mirror45.py: the box engine with both mirrors solving into
a caller's table, a torch.uint8 tensor of 2^32 bytes adopted as bench.py does (torch imported and
initialised first, then the library).  For each root given in hex on the command line: the table
is filled with 0xEE, the root solved, and one JSON line printed with the boxes that hold any other
byte, whether each of those is stored whole, the boxes that are not computed, and those of them
that differ from their computed representative under the row permutation of their mirrors."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gamesmanmpi_amd import Context, _lib  # noqa: E402
from test_box_mirror import box_index_of_key, in_region  # noqa: E402
from test_box_mirror45 import representative  # noqa: E402


def main():
    table = torch.empty(1 << 32, dtype=torch.uint8, device="cuda")
    boxes = table.view(1 << 20, 4096)
    for root in (int(a, 16) for a in sys.argv[1:]):
        table.fill_(0xEE)
        torch.cuda.synchronize()
        ctx = Context(_lib.GAME_SUBTRACT, (8,), device=0)
        ctx.adopt_dense_table(table.data_ptr(), table.numel())
        n, rec = ctx.solve(root)
        res, bad = ctx.verify()
        rb = box_index_of_key(root) >> 12
        touched = torch.nonzero((boxes != 0xEE).any(dim=1)).flatten().cpu().tolist()
        whole = all(bool((boxes[b] != 0xEE).all()) for b in touched)
        not_computed, differ = [], []
        for b in touched:
            if not in_region(b, rb):
                continue
            c, m67, m45 = representative(b, rb)
            if c == b:
                continue
            not_computed.append(b)
            rows = boxes[c].view(256, 4, 4)
            if m67:
                rows = rows[:, [0, 2, 1, 3], :]
            if m45:
                rows = rows[:, :, [0, 2, 1, 3]]
            if not torch.equal(boxes[b].view(256, 4, 4), rows):
                differ.append(b)
        ctx.close()
        print(json.dumps({"root": root, "n": n, "rec": rec, "touched": touched, "whole": whole,
                          "not_computed": not_computed, "differ": differ, "n_bad": res["n_bad"],
                          "checked": res["checked"]}), flush=True)


if __name__ == "__main__":
    main()
