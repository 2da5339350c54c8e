"""Writes tests/golden/layout_launches_parent.json: per layout and frame size the launch counts and the digests that
tests/test_gpu_layouts.py pins, as the checked-out tree gives them on the GPU.  It was run at the commit before the flat, gray
and channel-stride paths were put behind one host path; run it again only at a commit whose launches are the intended ones.
It needs the library built (python -m tezip_amd.build) and a GPU.

    python tests/golden/make_layout_launches.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]

if __name__ == "__main__":
    import test_gpu_layouts as T
    with open(T.FIXTURE, "w") as f:
        json.dump({"%s-%s" % c: T.record(*c) for c in T.CASES}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", T.FIXTURE)
