"""Writes tests/golden/scene_images_parent.json: for every valid case of tests/scene_device_cases.py, under both walk trees, what the getters
expose of rt_scene_create_ex's scene: rt_scene_get_info, and one SHA-256 each of rt_scene_get_filter_tree and rt_scene_get_walk_tree.  Run it
on the commit BEFORE csrc/rt_scene_plan.h existed (the parent of the commit that added this file), with that commit's library built and this
file and tests/scene_device_cases.py copied in: the fixture then holds the host code, which now computes every record through the shared
header, to the scenes the unrefactored code made.

    python tests/golden/make_scene_images_parent.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import scene_device_cases as sc  # noqa: E402


def main():
    out = {}
    for name, make in sc.CASES.items():
        records, textures = make()
        for walk in ("sah", "reference"):
            code, scene, text = sc.create("rt_scene_create_ex", records, textures, walk)
            assert code == 0, (name, walk, text)
            out[f"{name}/{walk}"] = sc.scene_record(scene)
    with open(os.path.join(HERE, "scene_images_parent.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} scenes")


if __name__ == "__main__":
    main()
