"""The bi-head graph with the operand rounding of the OPT-IN reduced-precision forward (OFX_OPT_POLICY_BF16: lowp 1 =
bf16, 2 = fp16 operands, fp32 sums), in torch CPU ops like tests/policy_ref64.py.  Test infrastructure, and the
written statement of WHICH operands that switch rounds (include/ofx.h points here):

  BatchNorm fold   in float32, as k_policy_prepare does it (inv = gamma / sqrtf(var + 1e-3f); kernel * inv;
                   b * inv + (beta - mean * inv), contracted to FMAs as that unit is built); then cast to `dtype`
  conv1            unrounded (table look-up of the bit maps)
  conv2 .. conv4   the layer's INPUT activations and its folded KERNEL rounded to nearest even; folded bias, sum,
                   ReLU and 2x2 max-pool unrounded - a layer's output is rounded only as the next 16-bit layer's input,
                   conv4's output enters dense1 unrounded.  Only the STREAMING trunk has a 16-bit form: the unfused
                   trunk (OFX_OPT_TRUNK_FUSE = 2, or auto with a small batch) stays fp32 - trunk_lowp=False
  dense1, dense2, output1, updense1, upconv1, upconv2    unrounded
  upconv3          in PHASE FORM on the 100 x 100 grid: for output parity (a, b) the 3 x 3 x 4 x 8 phase weights are the
                   float32 sum over (dy, dx), in that order, of folded * (up_coef(a, dy, ty) * up_coef(b, dx, tx)) (one
                   FMA per term, k_policy_prepare's w3mf); the PHASE WEIGHTS and the uprelu2 VALUES are rounded, bias and
                   sum are not.  Rows and columns 0 and 199 of uprelu3 (the frame lines, where zero padding and the
                   clamp-extended phase form differ) are the unrounded declared layer's (k_head_frames)
  upconv4          unrounded, its up-sampling included (the 1x1 on the fp32 matrix instruction, the stencil on the VALU)

With lowp = 0 this is tests/policy_ref64.forward up to the float32 fold (tests/test_policy_lowp_ref.py).  Evaluated
in float32 it is the YARDSTICK: the error an fp32 evaluation of the very same rounded graph has against the float64
one - operands that sit within fp32 error of a 16-bit rounding boundary resolve differently and move a few pixels by
a 16-bit ulp's worth; everything else agrees at the fp32 level.  The float32 evaluation runs in a written-down order of
elementwise operations (conv_fixed, dense_fixed, upsample2_fixed), so that WHICH operands flip - and with them every
figure the tests derive from the yardstick - does not depend on the machine's thread count or instruction set.
_mutate is private to the tests: three defects a looser comparison cannot see."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.policy_ref64 import _tensors, upsample2

LOWP_DTYPE = {1: torch.bfloat16, 2: torch.float16}
BN_LAYERS = ("conv1", "conv2", "conv3", "conv4", "upconv1", "upconv2", "upconv3")
MUTANTS = ("conv3_truncate", "conv4_unrounded", "upconv3_round_before_phase")

# up_coef of k_policy_prepare: output row 2 i + a, conv tap dy touches low-res rows i - 1, i, i + 1 with these weights
_UP = {False: (((0.75, 0.25, 0.0), (0.25, 0.75, 0.0), (0.0, 0.75, 0.25)), ((0.25, 0.75, 0.0), (0.0, 0.75, 0.25), (0.0, 0.25, 0.75))),
       True: (((0.5, 0.5, 0.0), (0.0, 1.0, 0.0), (0.0, 0.5, 0.5)), ((0.0, 1.0, 0.0), (0.0, 0.5, 0.5), (0.0, 0.0, 1.0)))}


def round_lowp(x, lowp):
    """Round to nearest even to bf16 (1) / fp16 (2) and back; 0: unchanged."""
    if not lowp:
        return x
    return x.to(torch.float32).to(LOWP_DTYPE[lowp]).to(x.dtype)


def truncate_bf16(x):
    """The conv3_truncate mutant: drop the low 16 bits of the float32 instead of rounding."""
    bits = x.to(torch.float32).contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(x.dtype)


def _fma32(a, b, c):
    """fl32(a * b + c) on float32 arrays: the product of two float32 is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def fold(w):
    """BatchNorm folded into kernel and bias in float32: {layer: (kernel [3][3][ci][co], bias [co])} as numpy float32."""
    T = {k: v.numpy() for k, v in _tensors(w, torch.float32).items()}
    out = {}
    for name in BN_LAYERS:
        inv = T[name + ".gamma"] / np.sqrt(T[name + ".var"] + np.float32(1e-3))
        assert inv.dtype == np.float32
        bias = _fma32(T[name + ".bias"], inv, _fma32(-T[name + ".mean"], inv, T[name + ".beta"]))
        out[name] = (T[name + ".kernel"] * inv, bias)
    return out


def phase_weights(kf, legacy=False):
    """w3mf of k_policy_prepare from the folded float32 kernel [3][3][ci][co]: [a][b][ty][tx][ci][co], float32."""
    C = np.asarray(_UP[bool(legacy)], np.float32)
    out = np.zeros((2, 2, 3, 3) + kf.shape[2:], np.float32)
    for a in range(2):
        for b in range(2):
            for ty in range(3):
                for tx in range(3):
                    acc = np.zeros(kf.shape[2:], np.float32)
                    for dy in range(3):
                        for dx in range(3):
                            acc = _fma32(kf[dy, dx], np.broadcast_to(C[a, dy, ty] * C[b, dx, tx], acc.shape), acc)
                    out[a, b, ty, tx] = acc
    return out


def conv_fixed(x, k, b, pad=1):
    """conv3x3 on NCHW, HWIO kernel, in a WRITTEN-DOWN order of elementwise operations: bias, then for every tap (dy, dx)
    and input channel in turn one rounded product and one rounded sum.  No library reduction: the float32 result is the
    same bits on every machine, whatever the thread count or the instruction set."""
    xp = F.pad(x, (pad, pad, pad, pad)) if pad else x
    H, W = xp.shape[-2] - 2, xp.shape[-1] - 2
    out = b.view(1, -1, 1, 1).expand(x.shape[0], -1, H, W).clone()
    for dy in range(3):
        for dx in range(3):
            for ci in range(k.shape[2]):
                out += xp[:, ci:ci + 1, dy:dy + H, dx:dx + W] * k[dy, dx, ci].view(1, -1, 1, 1)
    return out


def dense_fixed(a, k, b, chunk=313):
    """a [K][n] @ k [n][m] + b in a written-down order: partial sums over chunks of 313 inputs (5008 = 16 x 313), each
    accumulated term by term, then the partials and the bias in turn."""
    parts = []
    for s in range(0, a.shape[1], chunk):
        acc = torch.zeros(a.shape[0], k.shape[1], dtype=a.dtype)
        for j in range(s, min(s + chunk, a.shape[1])):
            acc += a[:, j:j + 1] * k[j:j + 1]
        parts.append(acc)
    out = parts[0]
    for q in parts[1:]:
        out = out + q
    return out + b


def upsample2_fixed(u, legacy=False):
    """upsample2 as an explicit gather and one a * wa + b * wb per axis (two rounded products, one rounded sum)."""
    n = u.shape[-1]
    k = torch.arange(2 * n)
    if legacy:      # out[2m] = in[m], out[2m+1] = (in[m] + in[m+1]) / 2
        i0, i1, w1 = k // 2, torch.clamp(k // 2 + 1, max=n - 1), (k % 2) * 0.5
    else:           # out[2m] = .25 in[m-1] + .75 in[m], out[2m+1] = .75 in[m] + .25 in[m+1]
        i0, i1 = torch.clamp((k - 1) // 2, min=0), torch.clamp((k + 1) // 2, max=n - 1)
        w1 = 0.75 - 0.5 * (k % 2)
    w1 = w1.to(u.dtype)
    u = u[..., i0, :] * (1 - w1)[:, None] + u[..., i1, :] * w1[:, None]
    return u[..., :, i0] * (1 - w1) + u[..., :, i1] * w1


def forward(sm, lm, vec8s, w, lowp, dtype=torch.float64, legacy_bilinear=False, trunk_lowp=True, head_lowp=True,
            _mutate=None, _probe=None, fixed_order=None):
    """One arena: maps (400,400) uint8, vec8s [K][8] heads of K ships -> act [K][2], heat [K][400][400] (numpy, dtype).
    _probe: a dict that receives the activations in front of their rounding ("conv2" .. "conv4" [8][H][W], "upconv3"
    [K][4][100][100]) for boundary_distance.
    fixed_order (default: for float32): every sum in the written-down order of conv_fixed / dense_fixed / upsample2_fixed
    instead of the libraries' - the float32 YARDSTICK must not depend on the machine it runs on, or the bounds derived
    from it would; in float64 the order moves nothing a 16-bit rounding can see."""
    if fixed_order is None:
        fixed_order = dtype == torch.float32
    assert lowp in (0, 1, 2) and _mutate in (None,) + MUTANTS
    T = _tensors(w, dtype)
    Fd = {k: (torch.from_numpy(kk).to(dtype), torch.from_numpy(bb).to(dtype)) for k, (kk, bb) in fold(w).items()}
    rnd = lambda t: round_lowp(t, lowp)

    def conv(x, k, b, pad=1):                       # HWIO -> OIHW
        return conv_fixed(x, k, b, pad) if fixed_order else F.conv2d(x, k.permute(3, 2, 0, 1), b, padding=pad)

    def dense(a, name):
        k, b = T[name + ".kernel"], T[name + ".bias"]
        return dense_fixed(a, k, b) if fixed_order else a @ k + b

    up2 = upsample2_fixed if fixed_order else upsample2

    x = torch.from_numpy(np.stack([sm, lm], 0).astype(np.float64)).to(dtype)[None]   # NCHW
    for i in (1, 2, 3, 4):
        k, b = Fd["conv%d" % i]
        if i > 1 and trunk_lowp and lowp:
            if _probe is not None:
                _probe["conv%d" % i] = x[0].numpy().copy()
            if _mutate == "conv3_truncate" and i == 3:
                x, k = truncate_bf16(x), truncate_bf16(k)
            elif not (_mutate == "conv4_unrounded" and i == 4):
                x, k = rnd(x), rnd(k)
        x = F.max_pool2d(F.relu(conv(x, k, b)), 2)
    flat = x.permute(0, 2, 3, 1).reshape(1, -1)                                        # Flatten (h, w, c)
    v = torch.from_numpy(np.asarray(vec8s, np.float64)).to(dtype)
    cat = torch.cat([v, flat.expand(v.shape[0], -1)], 1)                               # vector first
    d1 = F.relu(dense(cat, "dense1"))
    d2 = F.relu(dense(d1, "dense2"))
    act = dense(d2, "output1")
    u = F.relu(dense(d1, "updense1")).reshape(-1, 1, 25, 25)
    for i in (1, 2):
        u = F.relu(conv(up2(u, legacy_bilinear), *Fd["upconv%d" % i]))
    # upconv3: the declared layer (its frame lines are the kernel's), then the phase form over it everywhere else
    k3, b3 = Fd["upconv3"]
    u3 = F.relu(conv(up2(u, legacy_bilinear), k3, b3))
    k3f = fold(w)["upconv3"][0]
    if _mutate == "upconv3_round_before_phase" and head_lowp and lowp:
        pw = torch.from_numpy(phase_weights(rnd(torch.from_numpy(k3f)).numpy(), legacy_bilinear)).to(dtype)
    else:
        pw = torch.from_numpy(phase_weights(k3f, legacy_bilinear)).to(dtype)
        if head_lowp:
            pw = rnd(pw)
    if _probe is not None and head_lowp and lowp:
        _probe["upconv3"] = u.numpy().copy()
    up = F.pad(rnd(u) if head_lowp else u, (1, 1, 1, 1), mode="replicate")          # the clamp-extended low-res plane
    ph = torch.empty_like(u3)
    for a in range(2):
        for b in range(2):
            ph[:, :, a::2, b::2] = F.relu(conv(up, pw[a, b], b3, pad=0))
    ph[:, :, 0, :], ph[:, :, -1, :], ph[:, :, :, 0], ph[:, :, :, -1] = u3[:, :, 0, :], u3[:, :, -1, :], u3[:, :, :, 0], u3[:, :, :, -1]
    heat = conv(up2(ph, legacy_bilinear), T["upconv4.kernel"], T["upconv4.bias"])[:, 0]
    return act.numpy(), heat.numpy()


def boundary_distance(x, lowp):
    """(distance of x to the nearest 16-bit rounding boundary) / |x|; inf for x = 0.  An operand whose distance is within
    the fp32 error of its evaluation (a few 1e-7) can round either way.  Diagnostic: the quantum is taken at the rounded
    value, so the figure is off by up to a factor 2 right at a power of two."""
    x = np.asarray(x, np.float64)
    r = round_lowp(torch.from_numpy(x.copy()), lowp).numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.abs(r)))
        quantum = 2.0 ** (e - 7) if lowp == 1 else 2.0 ** (np.maximum(e, -14) - 10)
        d = np.abs(quantum / 2 - np.abs(x - r)) / np.abs(x)
    d[(x == 0) | (r == 0)] = np.inf
    return d


def stats(act, heat, act64, heat64, tol_heat):
    """Per ship, normalised as policy_ref64.errors: act error; over the heat map's interior and over its frame the share of
    pixels beyond tol_heat and the max error; p99 over the whole map; the worst pixel (y, x)."""
    from tests.policy_ref64 import frame_mask
    fm = frame_mask()
    e = np.abs(np.asarray(heat, np.float64) - heat64) / float(np.abs(heat64).max())
    y, x = np.unravel_index(int(np.argmax(e)), e.shape)
    return dict(act=float(np.abs(np.asarray(act, np.float64) - act64).max() / max(1.0, np.abs(act64).max())),
                share=float((e > tol_heat).sum()) / e.size, share_interior=float((e[~fm] > tol_heat).sum()) / e.size,
                share_frame=float((e[fm] > tol_heat).sum()) / e.size, max=float(e.max()), max_interior=float(e[~fm].max()),
                max_frame=float(e[fm].max()), p99=float(np.percentile(e, 99)), worst=(int(y), int(x)))
