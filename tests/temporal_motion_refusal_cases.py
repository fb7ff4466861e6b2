"""What the motion calls of the temporal accumulator refuse (include/ptcore.h, "moving spheres"), as data: shared by
test_temporal_motion_host.py (pt_temporal_scene_check, which needs neither a device nor a session) and
test_temporal_motion_gpu.py (the same arguments through a live session, whose state must survive the refusal).

A case is (name, edit, word): edit(now, prev, basis, eye) changes the good arguments in place or returns replacements as a dict
with the keys "now", "prev", "n", "basis", "eye" (None: a null pointer); word must appear in the message next to PT_EINVAL."""
import numpy as np

PT_EINVAL = -1


def _set(field, index, value, which="now", component=None):
    def edit(now, prev, basis, eye):
        a = now if which == "now" else prev
        if component is None:
            a[field][index] = value
        else:
            a[field][index, component] = value
    return edit


def _basis(change):
    def edit(now, prev, basis, eye):
        change(basis)
    return edit


def _flat(b):
    b[3:6] = b[0:3]  # B1 = B0: no width


def _skew(b):
    b[9] += 0.01 * float(np.linalg.norm(b[0:3]))


def _nan(b):
    b[4] = np.nan


CASES = [
    ("n-zero", lambda *a: dict(n=0), "n 0 outside 1 .. 65535"),
    ("n-negative", lambda *a: dict(n=-4), "n -4 outside"),
    ("n-65536", lambda *a: dict(n=65536), "n 65536 outside"),
    ("null-now", lambda *a: dict(now=None), "null h_now"),
    ("null-prev", lambda *a: dict(prev=None), "null h_prev"),
    ("null-basis", lambda *a: dict(basis=None), "null basis"),
    ("null-eye", lambda *a: dict(eye=None), "null eye"),
    ("nan-pos-now", _set("pos", 4, np.nan, "now", 1), "h_now: pos[1] of sphere 4 is not finite"),
    ("inf-pos-prev", _set("pos", 8, np.inf, "prev", 2), "h_prev: pos[2] of sphere 8 is not finite"),
    ("nan-radius", _set("radius", 0, np.nan, "now"), "h_now: radius of sphere 0 is not finite"),
    ("inf-emission", _set("emission", 6, -np.inf, "prev", 0), "h_prev: emission[0] of sphere 6 is not finite"),
    ("nan-color", _set("color", 2, np.nan, "now", 2), "h_now: color[2] of sphere 2 is not finite"),
    ("radius-changed", _set("radius", 7, 16.0, "now"), "reset the session"),
    ("radius-one-ulp", _set("radius", 8, float(np.nextafter(np.float32(16.5), np.float32(17.0))), "prev"), "radius of sphere 8"),
    ("radius-minus-zero", lambda now, prev, b, e: (now["radius"].__setitem__(3, 0.0), prev["radius"].__setitem__(3, -0.0)) and None,
     "radius of sphere 3"),
    ("nan-eye", lambda now, prev, b, eye: eye.__setitem__(1, np.nan), "eye[1] is not finite"),
    ("basis-flat", _basis(_flat), "determinant"),
    ("basis-skew", _basis(_skew), "parallelogram"),
    ("basis-nan", _basis(_nan), "determinant"),
]
IDS = [c[0] for c in CASES]


def arguments(pt, edit, width=64, height=64):
    """(now, prev, n, basis, eye) for the C ABI after `edit`: numpy arrays or None, n an int."""
    now = pt.scene_cornell()
    prev = now.copy()
    prev["pos"][7] -= np.float32(1.5)
    basis = pt.camera_basis(width=width, height=height).copy()
    eye = np.array(pt.DEFAULT_EYE, np.float32)
    args = dict(now=now, prev=prev, n=len(now), basis=basis, eye=eye)
    args.update(edit(now, prev, basis, eye) or {})
    return args


def pointer(a, ctype=None):
    import ctypes
    if a is None:
        return None
    return a.ctypes.data if ctype is None else a.ctypes.data_as(ctypes.POINTER(ctype))
