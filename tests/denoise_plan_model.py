"""The denoiser's layer table and plan rule (csrc/pt_denoise.hip: build_layers, pick_cfg, choose_tiles, batch_plan) restated in
Python, so that what a test case claims about a plan -- this tile shape, that many K slices, a ragged last tile -- can be
checked without a device, and so that the GPU tests can hold the library's own conv_plan(g) to it field by field.  The
constants (kCfg, kPlan, kChannels, BK, XC) are read from the source text: a changed table changes the model with it, and the
case table's reasons (tests/denoise_group_cases.py) then fail on the CPU instead of going blind on the GPU.

The rule.  A layer of N columns and M rows takes the wide tile of its column class (N <= 32: kCfg[0], N <= 64: kCfg[1], else
kCfg[2]) when it fills at least wide_tiles[class] of them, else the small one (kCfg[3] for N <= 32, else kCfg[4]).  K = taps x
stored Cin is cut into 16-wide chunks; a layer of fewer than target_wgs / 2 tiles is split into ceil(target_wgs / tiles)
slices, at most nchunks / min_chunks (at least 1), of ceil(nchunks / slices) chunks each.  A group of g frames has M = g rows
per output pixel, re-chooses the tile for that M (only among tiles whose width divides the single-frame column padding) and
KEEPS the single-frame K slicing."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-pathtrace_amd", "csrc")
EPI_ACT, EPI_LAT, EPI_RGB = 0, 1, 2
PRECISIONS = ("float32", "half")


def _source():
    return open(os.path.join(CSRC, "pt_denoise.hip")).read()


def _ints(text):
    return [int(v) for v in re.findall(r"-?\d+", text)]


def constants(text=None):
    """{"BK", "XC", "kChannels", "kCfg": [(bm, bn)] * 5, "kPlan": {precision: (wide_tiles[3], target_wgs, min_chunks)}}."""
    text = text or _source()
    out = {}
    for name in ("BK", "XC"):
        m = re.search(r"^constexpr int %s = (\d+);" % name, text, re.M)
        assert m, name
        out[name] = int(m.group(1))
    m = re.search(r"const int kChannels\[7\] = \{([^}]*)\};", text)
    assert m, "kChannels"
    out["kChannels"] = _ints(m.group(1))
    m = re.search(r"static const TileCfg kCfg\[5\] = \{(.*)\};", text)
    assert m, "kCfg"
    v = _ints(m.group(1))
    out["kCfg"] = [(v[2 * i], v[2 * i + 1]) for i in range(5)]
    m = re.search(r"static const PlanRule kPlan\[2\] = \{(.*)\};", text)
    assert m, "kPlan"
    v = _ints(m.group(1))
    assert len(v) == 10 and len(out["kCfg"]) == 5 and len(out["kChannels"]) == 7, (v, out)
    out["kPlan"] = {p: (tuple(v[5 * i:5 * i + 3]), v[5 * i + 3], v[5 * i + 4]) for i, p in enumerate(PRECISIONS)}
    return out


C = constants()


def ceil_div(a, b):
    return -(-a // b)


def tiles(M, N, cfg):
    bm, bn = C["kCfg"][cfg]
    return ceil_div(M, bm) * ceil_div(N, bn)


def pick_cfg(M, N, precision):
    wide = C["kPlan"][precision][0]
    if N <= 32:
        return 0 if tiles(M, N, 0) >= wide[0] else 3
    if N <= 64:
        return 1 if tiles(M, N, 1) >= wide[1] else 4
    return 2 if tiles(M, N, 2) >= wide[2] else 4


def levels(width, height):
    """[(rows, cols)] of the seven levels of the encoder."""
    out = [(height, width)]
    for _ in range(6):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def layers(width, height):
    """([(activation name, (rows, cols, channels))], [conv dict]) in execution order, one frame, no plan yet."""
    lv = levels(width, height)
    acts, convs = [], []

    def act(name, hw, c):
        acts.append((name, (hw[0], hw[1], c)))
        return len(acts) - 1

    def conv(name, src, ks, stride, N, epi, out0, out1=-1, res=-1, up=-1):
        ih, iw, cin = acts[src][1]
        oh, ow = (ih - 1) // stride + 1, (iw - 1) // stride + 1
        convs.append({"name": name, "in": src, "out0": out0, "out1": out1, "res": res, "up": up, "ks": ks, "stride": stride, "N": N,
                      "epi": epi, "cin": cin, "in_shape": acts[src][1], "out_h": oh, "out_w": ow, "out_hw": oh * ow,
                      "K": ks * ks * cin, "up_shape": acts[up][1] if up >= 0 else None})

    raw = [act("input", lv[0], C["XC"])]
    for b in range(1, 7):
        ch = C["kChannels"][b]
        t1, rs = act(f"block{b}.t1", lv[b], ch), act(f"block{b}.res", lv[b], ch)
        raw.append(act(f"block{b}.out", lv[b], ch))
        conv(f"block{b}.conv1+res_conv", raw[b - 1], 3, 2, 2 * ch, EPI_ACT, t1, out1=rs)
        conv(f"block{b}.conv2", t1, 3, 1, ch, EPI_ACT, raw[b], res=rs)
    rep = act("lat6", lv[6], 32)
    conv("lat_6", raw[6], 1, 1, 32, EPI_ACT, rep)
    for k in range(5, -1, -1):
        rh, rw, _ = acts[rep][1]
        bk = act(f"back{k + 1}{k}", ((rh + 1) // 2, (rw + 1) // 2), 32)
        conv(f"backwards_{k + 1}{k}", rep, 3, 2, 32, EPI_ACT, bk)
        nr = act(f"rep{k}", lv[k], 32)
        conv(f"lat_{k}", raw[k], 1, 1, 32, EPI_LAT, nr, up=bk)
        rep = nr
    conv("rgb_conv", rep, 3, 1, 3, EPI_RGB, -1)
    return acts, convs


def plan(width, height, precision, frames=1):
    """[conv dict + {"M", "bm", "bn", "splits", "chunks_per_split", "nchunks", "npad", "workgroups"}] of a group of `frames`."""
    _, target, min_chunks = C["kPlan"][precision]
    out = []
    for c in layers(width, height)[1]:
        c = dict(c)
        cfg = pick_cfg(c["out_hw"], c["N"], precision)
        npad = ceil_div(c["N"], C["kCfg"][cfg][1]) * C["kCfg"][cfg][1]
        nchunks = c["K"] // C["BK"]
        t = tiles(c["out_hw"], c["N"], cfg)
        splits = 1
        if t < target // 2:
            splits = min(ceil_div(target, t), max(nchunks // min_chunks, 1))
        cps = ceil_div(nchunks, splits)
        splits = ceil_div(nchunks, cps)
        M = frames * c["out_hw"]
        if frames > 1:
            again = pick_cfg(M, c["N"], precision)
            if npad % C["kCfg"][again][1] == 0:
                cfg = again
        bm, bn = C["kCfg"][cfg]
        c.update(M=M, bm=bm, bn=bn, splits=splits, chunks_per_split=cps, nchunks=nchunks, npad=npad,
                 workgroups=ceil_div(M, bm) * (npad // bn) * splits)
        out.append(c)
    return out


PLAN_FIELDS = ("M", "bm", "bn", "splits", "chunks_per_split", "workgroups")


def workspace_elements(width, height, frames, precision):
    """Elements of the activation workspace for groups of `frames` frames (layout_acts: every buffer 256-byte aligned), and
    the split-K partials in floats (partial_floats_of)."""
    al = 256 // (2 if precision == "half" else 4)
    ws = sum(ceil_div(frames * h * w * c, al) * al for _, (h, w, c) in layers(width, height)[0])
    part = max([c["splits"] * c["M"] * c["npad"] for c in plan(width, height, precision, frames) if c["splits"] > 1] or [0])
    return ws, part
