"""Child process of tests/test_gpu_box_mirror.py: the box engine solving into a caller's table,
a torch.uint8 tensor of 2^32 bytes adopted as bench.py does (torch imported and initialised
first, then the library).  For each root given in hex on the command line: the table is filled
with 0xEE, the root solved, and one JSON line printed with the boxes that hold any other byte,
whether each of those is stored whole, and the mirrored-to boxes that differ from their twin with
dwords 1 and 2 of every row exchanged."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gamesmanmpi_amd import Context, _lib  # noqa: E402
from test_box_mirror import box_index_of_key, in_region, mirror_class, swap67  # noqa: E402


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
        mirrored, differ = [], []
        for b in touched:
            if in_region(b, rb) and mirror_class(b, rb) == 2:
                mirrored.append(b)
                twin = boxes[swap67(b)].view(256, 4, 4)[:, [0, 2, 1, 3], :]
                if not torch.equal(boxes[b].view(256, 4, 4), twin):
                    differ.append(b)
        ctx.close()
        print(json.dumps({"root": root, "n": n, "rec": rec, "touched": touched, "whole": whole, "mirrored": mirrored,
                          "differ": differ, "n_bad": res["n_bad"], "checked": res["checked"]}), flush=True)


if __name__ == "__main__":
    main()
