"""Roofline numbers of the hand-off kernels at the sizes the reference runs them:
PSMNet volume for a 544x960 (padded 540x960) pair, maxdisp 192, 32 feature channels
(psmnet.py:157-197: [B,64,48,136,240] = 401 MB per frame in float32, 200 MB in bfloat16, write-bound), RAFT-Stereo
correlation modulation ([B,136,240,1,240]), KITTI payload decode.  --dtype picks the storage type of the two
volumes; with `both` (the default) the float32 call, the bfloat16 call and what a bfloat16 caller had to do before
there was one, psmnet_cost_volume(float32).to(bfloat16), are timed in one run, alternated round by round, and the two
conditions on the bfloat16 kernel are reported.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vppstereo_amd.engine import Engine  # noqa: E402
from tools._timing import alternate, timeit  # noqa: E402


def row(stat, bytes_written, **more):
    med, lo, hi = stat
    return dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), GB_written=round(bytes_written / 1e9, 3),
                write_GBps=round(bytes_written / med / 1e6, 1), **more)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--dtype", choices=("float32", "bfloat16", "both"), default="both")
    args = ap.parse_args()
    f32, bf16 = args.dtype in ("float32", "both"), args.dtype in ("bfloat16", "both")
    eng = Engine()
    dev = eng.device
    B, C, H4, W4, H, W, maxdisp = 4, 32, 136, 240, 544, 960, 192
    g = torch.Generator(device="cpu").manual_seed(1)
    fl = torch.randn((B, C, H4, W4), generator=g).to(dev)
    fr = torch.randn((B, C, H4, W4), generator=g).to(dev)
    valid = (torch.rand((B, 1, H, W), generator=g) < 0.03).float().to(dev)
    hints = (torch.rand((B, 1, H, W), generator=g) * 190 + 1).to(dev) * valid
    fl16, fr16 = fl.to(torch.bfloat16), fr.to(torch.bfloat16)
    out = {}
    cells = B * 2 * C * (maxdisp // 4) * H4 * W4
    variants = {}
    if f32:
        variants["float32"] = lambda: eng.psmnet_cost_volume(fl, fr, maxdisp, hints, valid)
    if bf16:
        variants["bfloat16"] = lambda: eng.psmnet_cost_volume(fl16, fr16, maxdisp, hints, valid)
    if f32 and bf16:
        variants["float32_then_cast"] = lambda: eng.psmnet_cost_volume(fl, fr, maxdisp, hints, valid).to(torch.bfloat16)
    stats = alternate(variants, rounds=9, iters=40, warm_iters=3, warm=2)
    written = {"float32": 4 * cells, "bfloat16": 2 * cells, "float32_then_cast": 6 * cells}
    psm = out["psmnet_cost_volume"] = {"frames": B, "shape": [B, 2 * C, maxdisp // 4, H4, W4], "rounds": 9, "iters_per_round": 40}
    for k, st in stats.items():
        psm[k] = row(st, written[k])
    if f32:     # the keys profiles/r01_handoff.json has
        psm.update(ms=psm["float32"]["ms"], GB_written=psm["float32"]["GB_written"], write_GBps=psm["float32"]["write_GBps"])
    if f32 and bf16:
        psm["condition_1_bf16_faster_than_float32"] = stats["bfloat16"][0] < stats["float32"][0]
        psm["condition_2_bf16_faster_than_float32_then_cast"] = stats["bfloat16"][0] < stats["float32_then_cast"][0]
        a = eng.psmnet_cost_volume(fl16, fr16, maxdisp, hints, valid)
        b = eng.psmnet_cost_volume(fl16.float(), fr16.float(), maxdisp, hints, valid).to(torch.bfloat16)
        psm["bf16_cells_unequal_to_float32_cast"] = int((a.float() != b.float()).sum().item())
        del a, b

    def torch_ref():  # what the reference executes (psmnet.py:157-197), same device
        cost = torch.zeros((B, 2 * C, maxdisp // 4, H4, W4), device=dev)
        for i in range(maxdisp // 4):
            if i > 0:
                cost[:, :C, i, :, i:] = fl[:, :, :, i:]
                cost[:, C:, i, :, i:] = fr[:, :, :, :-i]
            else:
                cost[:, :C, i] = fl
                cost[:, C:, i] = fr
        h = torch.nn.functional.interpolate(hints, size=[H // 4, W // 4], mode="nearest").squeeze(1)
        v = torch.nn.functional.interpolate(valid, size=[H // 4, W // 4], mode="nearest").squeeze(1)
        h = h * v / 4.0
        h = h.unsqueeze(1).unsqueeze(2).expand(-1, 2 * C, maxdisp // 4, -1, -1)
        v = v.unsqueeze(1).unsqueeze(2).expand(-1, 2 * C, maxdisp // 4, -1, -1)
        d = torch.linspace(0, maxdisp // 4 - 1, maxdisp // 4, device=dev).view(1, 1, -1, 1, 1).expand(B, 2 * C, -1, H4, W4)
        return cost * ((1 - v) + v * 10.0 * torch.exp(-(d - h) ** 2 / (2 * 0.25 ** 2)))
    if f32:
        ms_t = timeit(torch_ref, iters=3, warm=1)
        psm["torch_eager_ms"] = round(ms_t, 3)
        err = (eng.psmnet_cost_volume(fl, fr, maxdisp, hints, valid) - torch_ref()).abs().max().item()
        psm["max_abs_diff_vs_torch"] = err

    # in place and repeated: the values grow from call to call, the work does not depend on them
    corr = torch.randn((B, H4, W4, 1, W4), generator=g).to(dev)
    corr16 = corr.to(torch.bfloat16)
    variants = {}
    if f32:
        variants["float32"] = lambda: eng.raft_corr_modulate_(corr, hints, valid)
    if bf16:
        variants["bfloat16"] = lambda: eng.raft_corr_modulate_(corr16, hints, valid)
    stats = alternate(variants, rounds=9, iters=40, warm_iters=3, warm=2)
    rows = int((torch.nn.functional.interpolate(valid, size=[H4, W4], mode="nearest") != 0).sum().item())
    raft = out["raft_corr_modulate"] = {"frames": B, "rows_with_a_hint": rows, "rows": B * H4 * W4,
                                        "note": "in place, only rows with a hint are touched"}
    for k, st in stats.items():
        size = 4 if k == "float32" else 2
        raft[k] = row(st, rows * W4 * size, volume_GB=round(corr.numel() * size / 1e9, 3))
    if f32:
        raft.update(ms=raft["float32"]["ms"], volume_GB=raft["float32"]["volume_GB"])
    png = torch.randint(0, 65536, (64, 375, 1242), generator=g).to(torch.int16).to(dev)
    ms = timeit(lambda: eng.kitti_disp_decode(png), iters=10, warm=2)
    nb = png.numel() * (2 + 4 + 1)
    out["kitti_disp_decode"] = {"ms": round(ms, 4), "GBps": round(nb / ms / 1e6, 1), "frames": 64}
    # cfg 4: VPP only -> network tensors, device resident (17 B/pixel: latency bound)
    import synth
    for Bv in (1, 32):
        b = synth.make_batch(min(Bv, 4), 540, 960, 192, 0.03, seed=1234)
        idx = [i % min(Bv, 4) for i in range(Bv)]
        lt = torch.from_numpy(np.ascontiguousarray(b["left"][idx])).to(dev)
        rt = torch.from_numpy(np.ascontiguousarray(b["right"][idx])).to(dev)
        ht = torch.from_numpy(np.ascontiguousarray(b["hints"][idx])).to(dev)

        def vpp_to_net():
            lv, rv = eng.vpp(lt, rt, ht, seed=1)
            return eng.to_network_input(lv, torch.bfloat16), eng.to_network_input(rv, torch.bfloat16)
        ms = timeit(vpp_to_net, iters=10, warm=2)
        out[f"vpp_to_bf16_nchw_B{Bv}"] = {"ms": round(ms, 4), "us_per_frame": round(ms * 1e3 / Bv, 1)}
    out["device"] = eng.ctx.device_name
    print(json.dumps(out))


if __name__ == "__main__":
    main()
