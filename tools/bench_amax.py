import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hplflownet_amd import ops
for rows, cols in [(25841, 1024), (25841, 580), (34631, 512), (9433, 388)]:
    X = torch.randn(rows, cols, device='cuda')
    ops.amax(X); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(20): ops.amax(X)
    e.record(); torch.cuda.synchronize()
    t = s.elapsed_time(e) / 20
    assert float(ops.amax(X)) == float(X.abs().max())
    print(rows, cols, '%.1f us incl. clear  %.2f TB/s' % (t * 1e3, rows * cols * 4 / t / 1e9))
