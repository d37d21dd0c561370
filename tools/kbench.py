"""Per-kernel timing of the network kernels at the bench shapes (HIP events, many reps).  python tools/kbench.py"""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sample_factory_amd import lib

def desc(Cin, H, W, Cout, K, S, u8=0):
    return lib.sf_conv_desc(Cin=Cin, H=H, W=W, Cout=Cout, KH=K, KW=K, stride=S, OH=(H-K)//S+1, OW=(W-K)//S+1, in_u8=u8,
                            relu=1, traj_T=0, sub_mean=0.0, inv_scale=1/255.0 if u8 else 1.0)

LAYERS = [("conv1", desc(4,84,84,32,8,4,1)), ("conv2", desc(32,20,20,64,4,2)), ("conv3", desc(64,9,9,64,3,1)),
          ("fc", desc(3136,1,1,512,1,1)), ("heads", desc(512,1,1,8,1,1))]

def timeit(fn, reps):
    fn(); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps

def digest(t):  # KBENCH_HASH=1: seeded inputs + a digest of every result (bit-identity of two builds of the library)
    import hashlib
    return hashlib.sha1(t.detach().cpu().numpy().tobytes()).hexdigest()[:12]

def main():
    which = sys.argv[1:] or ["fwd", "wgrad", "dgrad"]
    HASH = os.environ.get("KBENCH_HASH") == "1"
    if HASH: torch.manual_seed(0)
    ns = [int(v) for v in os.environ["KBENCH_NS"].split(",")] if os.environ.get("KBENCH_NS") else [4096, 32768]
    only = os.environ.get("KBENCH_LAYERS", "").split(",") if os.environ.get("KBENCH_LAYERS") else None
    grads_at = set(ns) if os.environ.get("KBENCH_NS") else {32768}  # gradients: the training batch, or every n asked for
    for n in ns:
        for name, d in LAYERS:
            if only and name not in only: continue
            K = d.KH*d.KW*d.Cin
            M = n*d.OH*d.OW
            flops = 2.0*M*d.Cout*K
            if d.in_u8: x = torch.randint(0,256,(n,d.Cin,d.H,d.W),dtype=torch.uint8,device="cuda")
            else: x = torch.randn((n,d.H,d.W,d.Cin),device="cuda")
            w = torch.randn((K,d.Cout),device="cuda")/np.sqrt(K); b = torch.zeros(d.Cout,device="cuda")
            out = torch.empty((M,d.Cout),device="cuda"); dy = torch.randn((M,d.Cout),device="cuda")
            reps = 5 if n >= 32768 else (20 if n >= 4096 else 100)
            stride = d.Cin*d.H*d.W
            res = []
            if "fwd" in which:
                wsb = lib.conv_fwd_workspace(n, d); ws = torch.empty(max(wsb,16),dtype=torch.uint8,device="cuda") if wsb else None
                t = timeit(lambda: lib.conv_fwd(x, stride, None, 0, w, b, out, n, d, ws), reps); res.append(f"fwd {t*1e3:8.1f}us {flops/t/1e9:6.1f}TF" + (f" #{digest(out)}" if HASH else ""))
            if "fwd" in which and lib.conv_fwd_t_supported(n, d):
                wt = torch.empty((d.Cout, K), device="cuda"); lib.transpose(w, wt, K, d.Cout)
                assert torch.equal(wt, w.t().contiguous())
                ref = out.clone(); out.zero_()
                for cfg in os.environ.get("GLDS_CFGS", "0").split(","):
                    nb = lib.conv_fwd_t_workspace(n, d); wst = torch.empty(nb,dtype=torch.uint8,device="cuda") if nb else None
                    t = timeit(lambda: lib.conv_fwd_t(x, stride, wt, b, out, n, d, wst), reps)
                    err = (out - ref).abs().max().item() / ref.abs().max().item()
                    res.append(f"fwd_t {t*1e3:8.1f}us {flops/t/1e9:6.1f}TF relerr {err:.1e}" + (f" #{digest(out)}" if HASH else ""))
            if "fwd_os" in which and name in ("conv1", "conv2", "conv3"):
                # the rollout-size launch into slot t of a kept [n, T, pixels * channels] buffer (t walks the slots), reading its
                # input from such a buffer as well (conv2, conv3), against the dense launch of the same kernel; KBENCH_T slots
                T = int(os.environ.get("KBENCH_T", "32"))
                L_out, L_in = d.OH*d.OW*d.Cout, d.H*d.W*d.Cin
                kept = torch.empty((n, T, L_out), device="cuda"); step = [0]
                if d.in_u8:
                    mk = torch.empty((n, T, d.OH*d.OW), dtype=torch.int32, device="cuda"); mkd = torch.empty((M,), dtype=torch.int32, device="cuda")
                    def strided():
                        t_ = step[0] % T; step[0] += 1
                        lib.conv_fwd_relu_mask_os(x, stride, None, 0, w, b, kept[:, t_], T*L_out, mk[:, t_], T*d.OH*d.OW, n, d)
                    dense = lambda: lib.conv_fwd_relu_mask(x, stride, None, 0, w, b, out, mkd, n, d)
                else:
                    wt = torch.empty((d.Cout, K), device="cuda"); lib.transpose(w, wt, K, d.Cout)
                    xin = torch.randn((n, T, L_in), device="cuda")
                    def strided():
                        t_ = step[0] % T; step[0] += 1
                        lib.conv_fwd_t_os(xin[:, t_], T*L_in, wt, b, kept[:, t_], T*L_out, n, d)
                    dense = lambda: lib.conv_fwd_t(x, stride, wt, b, out, n, d)
                for rnd in range(2):
                    td, ts = timeit(dense, reps), timeit(strided, max(reps, T))
                    res.append(f"dense {td*1e3:8.1f}us strided(T={T}) {ts*1e3:8.1f}us")
            if "fwd_os2" in which and name in ("conv1", "conv2", "conv3", "fc"):
                # the two-segment twins (sf_conv_fwd_*_os2) at the rollout size, to tell the twin's address work from the scatter of
                # its kept segment: the dense launch (conv1: without sign-bit words, as the plain rollout runs it) | keep_n = 0 (the
                # dense segment alone: must time like the dense launch) | keep_n = n into T slots (today's strided launch) |
                # keep_n = n with T = 1 (the strided code writing contiguous memory: address work alone) | keep_n = n / 4 (the
                # headline split).  fc writes a dense output in every mode; only its input has the two segments.
                T = int(os.environ.get("KBENCH_T", "32"))
                L_out, L_in, P = d.OH*d.OW*d.Cout, d.H*d.W*d.Cin, d.OH*d.OW
                fc = name == "fc"
                kept = None if fc else torch.empty((n, T, L_out), device="cuda")
                step = [0]
                if d.in_u8:
                    mk = torch.empty((n, T, P), dtype=torch.int32, device="cuda")
                    dense = lambda: lib.conv_fwd(x, stride, None, 0, w, b, out, n, d, None)
                    def twin(kn, Tt):
                        t_ = step[0] % Tt; step[0] += 1
                        o1 = kept.view(-1)[:n*Tt*L_out].view(n, Tt, L_out); m1 = mk.view(-1)[:n*Tt*P].view(n, Tt, P)
                        lib.conv_fwd_relu_mask_os2(x, stride, None, 0, w, b, o1[:max(kn, 1), t_], Tt*L_out, m1[:max(kn, 1), t_], Tt*P,
                                                   out.view(n, L_out)[kn:] if kn < n else None, kn, n, d)
                else:
                    wt = torch.empty((d.Cout, K), device="cuda"); lib.transpose(w, wt, K, d.Cout)
                    xin = torch.randn((n, T, L_in), device="cuda")
                    x2 = x.view(n, L_in)
                    wst = None
                    if fc:
                        nb = lib.conv_fwd_t_workspace(n, d); wst = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
                    dense = lambda: lib.conv_fwd_t(x, stride, wt, b, out, n, d, wst)
                    def twin(kn, Tt):
                        t_ = step[0] % Tt; step[0] += 1
                        i1 = xin.view(-1)[:n*Tt*L_in].view(n, Tt, L_in)
                        if fc:
                            o1, oss = out.view(n, L_out), L_out
                        else:
                            o1, oss = kept.view(-1)[:n*Tt*L_out].view(n, Tt, L_out)[:, t_], Tt*L_out
                        lib.conv_fwd_t_os2(i1[:max(kn, 1), t_], Tt*L_in, x2[kn:] if kn < n else None, wt, b, o1[:max(kn, 1)], oss,
                                           out.view(n, L_out)[kn:] if kn < n else None, kn, n, d)
                for rnd in range(2):
                    r = max(reps, T)
                    res.append(f"dense {timeit(dense, r)*1e3:7.1f}us keep0 {timeit(lambda: twin(0, T), r)*1e3:7.1f}us "
                               f"keepN(T={T}) {timeit(lambda: twin(n, T), r)*1e3:7.1f}us keepN(T=1) {timeit(lambda: twin(n, 1), r)*1e3:7.1f}us "
                               f"keepN/4(T={T}) {timeit(lambda: twin(n // 4, T), r)*1e3:7.1f}us")
            if "wgrad" in which and n in grads_at:
                dw = torch.empty_like(w); db = torch.empty_like(b)
                ws = torch.empty(lib.conv_wgrad_workspace(n, d),dtype=torch.uint8,device="cuda")
                t = timeit(lambda: lib.conv_wgrad(x, stride, None, 0, dy, dw, db, n, d, ws), reps); res.append(f"wgrad {t*1e3:8.1f}us {flops/t/1e9:6.1f}TF" + (f" #{digest(dw)}" if HASH else ""))
            if "dgrad" in which and n in grads_at and not d.in_u8:
                din = torch.empty((n,d.H,d.W,d.Cin),device="cuda")
                t = timeit(lambda: lib.conv_dgrad(dy, w, x, din, n, d), reps); res.append(f"dgrad {t*1e3:8.1f}us {flops/t/1e9:6.1f}TF" + (f" #{digest(din)}" if HASH else ""))
            if "dgrad_noact" in which and n in grads_at and not d.in_u8:  # upper bound of what a mask-free epilogue could win
                din = torch.empty((n,d.H,d.W,d.Cin),device="cuda")
                t = timeit(lambda: lib.conv_dgrad(dy, w, None, din, n, d), reps); res.append(f"dgrad(no act read) {t*1e3:8.1f}us {flops/t/1e9:6.1f}TF" + (f" #{digest(din)}" if HASH else ""))
            print(f"n={n:6d} {name:6s} " + " | ".join(res), flush=True)

if __name__ == "__main__":
    main()
