"""What the GPU tests of the network-glue kernels share: sentinel cells around an output, float32 / bfloat16 tensors to
and from the device, and the comparison with a referee's namespace(value, limit).

TEST INFRASTRUCTURE ONLY.  torch is imported where it is used, so that collecting a GPU file needs none."""
import numpy as np

F32 = np.float32
SENTINEL32, SENTINEL16 = 0x7FA5A5A5, 0x7FA5      # NaN patterns no kernel here produces
GUARD = 8                                        # cells in front of and behind an output
INVALID, UNSUPPORTED = -1, -10
DTYPES = ("float32", "bfloat16")


def tdtype(dtype):
    import torch
    return torch.bfloat16 if dtype == "bfloat16" else torch.float32


def dev(eng, a, dtype="float32"):
    """A host float32 array on the device in the storage type `dtype` (a bfloat16 case holds bfloat16 values)."""
    import torch
    a = np.array(a, dtype=F32, order="C", copy=True)
    if dtype == "bfloat16":
        assert (a.view(np.uint32) & 0xFFFF == 0).all()
        return torch.from_numpy((a.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)).to(eng.device).view(torch.bfloat16)
    return torch.from_numpy(a).to(eng.device)


def host(t):
    """A device tensor of either dtype as float32 (exact)."""
    return t.float().cpu().numpy()


def bits(t):
    import torch
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def sentinels(eng, n, dtype):
    import torch
    it, val = (torch.int16, SENTINEL16) if dtype == "bfloat16" else (torch.int32, SENTINEL32)
    return torch.full((n,), val, dtype=it, device=eng.device)


def guarded(eng, shape, dtype, shift=0):
    """(buffer of sentinel cells, view of `shape` that starts GUARD + shift cells into it)."""
    n = int(np.prod(shape))
    buf = sentinels(eng, n + 2 * GUARD + shift, dtype)
    return buf, buf[GUARD + shift:GUARD + shift + n].view(tdtype(dtype)).view(*shape)


def guards_intact(buf, n, shift=0):
    raw = buf.cpu().numpy()
    val = SENTINEL16 if raw.dtype == np.int16 else SENTINEL32
    return bool((raw[:GUARD + shift] == val).all() and (raw[GUARD + shift + n:] == val).all())


def hold(R, got, ref, what, dtype="float32"):
    """R: the referee module whose compare / compare_bf16 judge `got`."""
    if dtype == "bfloat16":
        beyond, other = R.compare_bf16(got, ref)
        worst = float("nan")
    else:
        worst, beyond, other = R.compare(got, ref)
    print(f"{what} [{dtype}]: {got.size} cells ({int((R.classes(ref.value) != 0).sum())} not finite), worst |got - value| / limit "
          f"{worst:.3f}, {beyond} beyond, {other} of another class")
    assert other == 0, f"{what}: {other} cells are not of the referee's class"
    assert beyond == 0, f"{what}: {beyond} cells beyond the limit"
