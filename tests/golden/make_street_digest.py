"""Generate tests/golden/street_digest.json: a SHA-256 per procedural street scene over everything api.HostScene exposes of it.

Run on a build whose street is known good (the commit before a change to the host layer), from the repository root:
    python tests/golden/make_street_digest.py
tests/test_street_digest.py then holds every later build to the committed file: the GPU parity tests compare the GPU with the
oracle on whatever scene gfxh_scene_make_street hands them, so a changed street would pass them and still move every number measured
on it.  The digest covers, in this order, each array preceded by its length: counts; the bytes of every material; vertex bytes,
triangle bytes and material slot of every geometry instance; groups; instances with their transforms; width, height, format and
texels (or block format and blocks) of every texture.
"""
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "street_digest.json")

# name -> (function of gfxexp_amd.scenes, keyword arguments)
SCENES = {}
for _scale in (1, 2):
    for _tag, _kw in (("plain", {}), ("textured", {"textured": True}), ("cluttered", {"cluttered": True})):
        SCENES["small_street_seed7_scale%d_%s" % (_scale, _tag)] = ("small_street", dict(_kw, seed=7, scale=_scale))
for _tag, _kw in (("plain", {}), ("textured", {"textured": True}), ("cluttered", {"cluttered": True})):
    SCENES["bench_street_%s" % _tag] = ("bench_street", _kw)


def digest(scene):
    h = hashlib.sha256()

    def u32(*values):
        h.update(struct.pack("<%dI" % len(values), *values))

    def blob(data):
        data = bytes(data)
        h.update(struct.pack("<Q", len(data)))
        h.update(data)

    c = scene.counts()
    u32(c["materials"], c["geoms"], c["groups"], c["insts"], c["triangles"])
    for m in scene.materials():
        blob(m)
    for v, t, mat in scene.geoms():
        blob(v.tobytes())
        blob(t.tobytes())
        u32(mat)
    for g in scene.groups():
        blob(g.tobytes())
    for group, xfm in scene.instances():
        u32(group)
        blob(xfm.tobytes())
    textures = scene.textures()
    u32(len(textures))
    for t in textures:
        u32(*t[:4])
        if t[4] is None:
            u32(t[5])
            blob(t[6].tobytes())
        else:
            blob(t[4].tobytes())
    return h.hexdigest()


def scene_digest(name):
    from gfxexp_amd import scenes
    fn, kw = SCENES[name]
    return digest(getattr(scenes, fn)(**kw))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    out = {name: scene_digest(name) for name in SCENES}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)
    for name in sorted(out):
        print(name, out[name])
