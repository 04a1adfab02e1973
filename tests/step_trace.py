"""The fused step as the list of C calls it makes (a plain helper module, imported like exact_util).

``Recorder`` swaps the loaded library handle (``_lib._lib``) for a proxy that forwards every ``vg_*`` call and keeps
``[name, normalised arguments]``.  The normalisation makes a trace comparable across commits, processes and runs:

  integers, floats, seeds  as they are
  the stream argument      "s0" = the stream that was current when the recording began, "s1" = any other
  None                     None
  a device pointer         [allocation index, byte offset].  The allocations are the distinct storages of every tensor reachable
                           from the engine (its own buffers, both FlatParams, the SpectralState, the modules) and of the caller's
                           ``real`` / ``z``, and the host tables (ctypes arrays) found on the same walk - the SpectralState's
                           descriptor table is one, the C calls take it beside its device copy.  Plain integers, ``c_void_p``
                           and the pointer fields of a ``VgVitNet`` / ``VgGenNet`` passed by reference are all treated so.
                           Allocations are numbered by first appearance in the trace: no attribute name enters the fixture.
  any other pointer        "ext" (only ``sample()`` has such per-call temporaries; a traced step must have none)
  a struct                 field by field, in declaration order

``python tests/step_trace.py --write`` records every configuration of ``CONFIGS`` into tests/golden/step_trace.json;
tests/test_step_trace_gpu.py compares a fresh recording with it.
"""
import bisect
import ctypes as C
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:  # run as a script: the package is found like under pytest
    sys.path.insert(0, os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "golden", "step_trace.json")
B, STEPS = 4, 2
AUG = "color,translation,cutout"

# every branch of the single-process step at least once
CONFIGS = {
    "plain": {},
    "unfused": dict(fuse_real_fake=False),
    "two_stream": dict(two_stream=True),
    "two_stream_noise_ema": dict(two_stream=True, instance_noise=0.1, ema_decay=0.999),
    "instance_noise": dict(instance_noise=0.1),
    "wasserstein_clip_diversity": dict(loss="wasserstein", clip_d=5, clip_g=0.5, diversity_weight=0.1),
    "gp": dict(gp_weight=10),
    "diffaug": dict(diffaug=AUG),
    "diffaug_p": dict(diffaug=AUG, aug_p=0.5),
    "diffaug_ada": dict(diffaug=AUG, ada_target=0.6, ada_interval=2),
    "bcr_diffaug": dict(bcr=(10, 10), diffaug=AUG),
    "bcr_own_noise": dict(bcr=(10, 10), bcr_aug="translation", instance_noise=0.1),
    "spectral_all": dict(spectral_norm="all"),
    "ema": dict(ema_decay=0.999),
    "dense_top": dict(dense_top_block=True),
}
# an option that is off leaves the step launch for launch the plain one
OFF = {
    "diffaug_off": dict(diffaug=""),
    "ema_off": dict(ema_decay=0),
    "spectral_off": dict(spectral_norm=""),
    "bcr_off": dict(bcr=(0, 0)),
    "ada_off": dict(aug_p=None, ada_target=0),
}


def _lib():
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd import _lib as L
    return L


def _allocations(roots):
    """(base address, bytes) of every tensor storage and ctypes array reachable from ``roots``"""
    found, seen, todo = {}, set(), list(roots)
    while todo:
        o = todo.pop()
        if id(o) in seen or o is None or isinstance(o, (int, float, str, bytes, bool, type)):
            continue
        seen.add(id(o))
        if torch.is_tensor(o):
            s = o.untyped_storage()
            if s.nbytes():
                found[s.data_ptr()] = max(found.get(s.data_ptr(), 0), s.nbytes())
        elif isinstance(o, C.Array):
            found[C.addressof(o)] = C.sizeof(o)
        elif isinstance(o, dict):
            todo.extend(o.values())
        elif isinstance(o, (list, tuple, set)):
            todo.extend(o)
        elif hasattr(o, "__dict__") and not callable(o) or isinstance(o, torch.nn.Module):
            todo.extend(vars(o).values())
    return sorted(found.items())


class Recorder:
    """with Recorder(engine, real, z) as calls: engine.step(real, z) ...; ``calls`` is the trace, ``ext`` counts the foreign pointers"""

    def __init__(self, *roots):
        self.roots, self.calls, self.ext = roots, [], 0
        self.index = {}

    def __enter__(self):
        self.L = _lib()
        self.handle = self.L.lib()
        self.s0 = torch.cuda.current_stream().cuda_stream
        self.allocs = _allocations(self.roots)
        self.L._lib = self
        return self

    def __exit__(self, *exc):
        self.L._lib = self.handle

    def __getattr__(self, name):  # the proxy: what _lib.lib() hands out while the recording runs
        if name in ("handle", "L"):
            raise AttributeError(name)
        fn = getattr(self.handle, name)
        if not name.startswith("vg_"):
            return fn
        types = self.L._SIGNATURES[name][1]

        def call(*args):
            self.calls.append([name, self._args(args, types)])
            return fn(*args)
        return call

    def _find(self, addr):
        i = bisect.bisect_right(self.allocs, (addr, float("inf"))) - 1
        if i >= 0 and addr < self.allocs[i][0] + self.allocs[i][1]:
            return self.allocs[i][0]
        return None

    def _pointer(self, v):
        addr = v.value if isinstance(v, C.c_void_p) else v
        if not addr:
            return None
        base = self._find(addr)
        if base is None:  # allocated since the recording began (a lazily made buffer): look once more
            self.allocs = _allocations(self.roots)
            base = self._find(addr)
        if base is None:
            self.ext += 1
            return "ext"
        return [self.index.setdefault(base, len(self.index)), addr - base]

    def _struct(self, s):
        out = []
        for field, ftype in s._fields_:
            v = getattr(s, field)
            if isinstance(v, C.Structure):
                out.append(self._struct(v))
            elif ftype is C.c_void_p:
                out.append(self._pointer(v))
            else:
                out.append(list(v) if isinstance(v, C.Array) else v)
        return out

    def _args(self, args, types):
        out = []
        for i, (a, t) in enumerate(zip(args, types)):
            if t is C.c_void_p and i == len(types) - 1 and len(types) > 1:  # every enqueueing call ends with its stream
                s = (a.value if isinstance(a, C.c_void_p) else a) or 0
                out.append("s0" if s == self.s0 else "s1")
            elif t is C.c_void_p:
                out.append(self._pointer(a))
            elif hasattr(a, "_obj"):  # byref(struct)
                out.append(self._struct(a._obj))
            elif isinstance(a, C.Structure):
                out.append(self._struct(a))
            else:
                out.append(getattr(a, "value", a))
        return out


def engine(**kw):
    """The smallest shape the engine tests use: B = 4, E = 384, two blocks each, 32 x 32, the modules' default dropout, train mode"""
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    torch.manual_seed(5)
    D = ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, batch_size=B, transformer_blocks_count=2)).cuda().train()
    G = SirenGenerator(layers=2).cuda().train()
    gp = kw.get("gp_weight", 0)
    eng = GanEngine(D, G, batch=B, seed=77, external_noise=True, **kw)
    if gp:
        eng.gp_epsilon = torch.rand(B, 1, 1, 1, generator=torch.Generator().manual_seed(6)).cuda()
    return eng


def trace(**kw):
    """(calls, foreign pointers) of STEPS eager steps of the engine built with ``kw``, in the form json.load gives back"""
    eng = engine(**kw)
    g = torch.Generator().manual_seed(4)
    data = [((torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).cuda(), torch.randn(B, 1024, generator=g).cuda()) for _ in range(STEPS)]
    try:
        with Recorder(eng, data) as rec:
            for real, z in data:
                eng.step(real, z)
        torch.cuda.synchronize()
    finally:
        eng.close()
    return json.loads(json.dumps(rec.calls)), rec.ext


def dumps(doc):
    """one call per line: the fixture stays readable and its diffs small"""
    out = ["{", f' "commit": {json.dumps(doc["commit"])},', f' "ext_allowed": {doc["ext_allowed"]},', ' "traces": {']
    names = list(doc["traces"])
    for name in names:
        out.append(f"  {json.dumps(name)}: [")
        calls = doc["traces"][name]
        out.extend("   " + json.dumps(c, separators=(",", ":")) + ("," if i + 1 < len(calls) else "") for i, c in enumerate(calls))
        out.append("  ]" + ("," if name != names[-1] else ""))
    out += [" }", "}", ""]
    return "\n".join(out)


def main(argv):
    if argv[:1] != ["--write"]:
        raise SystemExit("usage: python tests/step_trace.py --write [commit id]   (records tests/golden/step_trace.json)")
    import subprocess
    commit = argv[1] if len(argv) > 1 else subprocess.run(["git", "-C", HERE, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    doc = {"commit": commit, "ext_allowed": 0, "traces": {}}
    for name, kw in CONFIGS.items():
        calls, ext = trace(**kw)
        if ext:
            raise SystemExit(f"{name}: {ext} pointers outside every known allocation")
        doc["traces"][name] = calls
        print(f"{name}: {len(calls)} calls", flush=True)
    with open(FIXTURE, "w") as f:
        f.write(dumps(doc))


if __name__ == "__main__":
    main(sys.argv[1:])
