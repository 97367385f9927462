"""One render of the 74-object particle scene (tests/_cases.py: cbox_particles) at 256 x 256, 16 samples per pixel, with the
particles as copies or as instances: kernel time, rays and the scene's device bytes as one JSON line.  Run each form in a fresh
process:  python tools/instance_render_rate.py copies | instances"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import srt_amd  # noqa: E402
from _cases import pt_scene  # noqa: E402
from soft_rendering_toolsets_amd import scenes  # noqa: E402

if __name__ == "__main__":
    form = sys.argv[1]
    s = pt_scene("cbox_particles")
    if form == "instances":
        s = scenes.share_meshes(s)
    pt = srt_amd.Pathtracer(0)
    pt.set_params(256, 256, 16, 8, True)
    pt.build_scene(s)
    pt.set_camera(s["camera"])
    pt.render_epoch(1, 0, 16)                  # warm-up: code objects, buffers
    pt.ray_count(reset=True)
    pt.kernel_time(True)
    img = pt.render_epoch(1, 0, 16)
    ms, launches = pt.kernel_time(False)
    rays, _ = pt.ray_count()
    import hashlib
    print(json.dumps({"form": form, "kernel_form": pt.kernel_form(), "kernel_ms": ms, "launches": launches, "rays": rays,
                      "mrays_per_s": rays / ms / 1e3 if ms else None, "image_sha256_16": hashlib.sha256(img.tobytes()).hexdigest()[:16],
                      "counts": pt.scene_counts()}))
    pt.close()
