"""A few Gram launches of one kind (for profilers and for comparing two builds' outputs).
usage: python scripts/one_gram.py [count [sym|ordered|fwd|fwdsym [N T d [DUMP_DIR]]]]      default: 3 sym 1024 64 7
DUMP_DIR: the last launch's K (and grad_k) as DUMP_DIR/<mode>_<N>_<T>_<d>_{K,grad_k}.npy"""
import sys, torch
import os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sigsvgd_amd.utils.synthetic import synthetic_inputs
from sigsvgd_amd import ops
dev=torch.device('cuda:0')
count = int(sys.argv[1]) if len(sys.argv)>1 else 3
mode = sys.argv[2] if len(sys.argv)>2 else 'sym'
N,T,d = (int(v) for v in sys.argv[3:6]) if len(sys.argv)>5 else (1024,64,7)
X,s=synthetic_inputs(N,T,d); X=X.to(dev)
run = {'sym': lambda: ops.gram_fwd_bwd(X,X,1.0,y_is_x=True), 'ordered': lambda: ops.gram_fwd_bwd(X,X,1.0),
       'fwd': lambda: (ops.gram_fwd(X,X,1.0),), 'fwdsym': lambda: (ops.gram_fwd(X,X,1.0,y_is_x=True),)}[mode]
for _ in range(count):
    out = run()
torch.cuda.synchronize()
if len(sys.argv)>6:
    import numpy as np
    os.makedirs(sys.argv[6], exist_ok=True)
    for name, t in zip(('K','grad_k'), out):
        np.save(os.path.join(sys.argv[6], f'{mode}_{N}_{T}_{d}_{name}.npy'), t.cpu().numpy())
