"""Writes tests/golden/huff_family_parent.json: the digests of every encode_file and the texts of every parse refusal of
tests/test_huff_family.py, as the checked-out tree gives them.  It was run at the commit before huff, huffr, keycoder and
keycoderg were put on common code, and again (adding the huffd entries alone) at the commit before huffd.py gave up its own
tokeniser and decode loop; run it again only at a commit whose formats and messages are the intended ones.

    python tests/golden/make_huff_family.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]

if __name__ == "__main__":
    from tezip_amd import build, huff, huffd, huffr, keycoder, keycoderg
    import test_huff_family as T
    build.build()
    mods = {"huff": huff, "huffr": huffr, "huffd": huffd, "keycoder": keycoder, "keycoderg": keycoderg}
    with open(T.FIXTURE, "w") as f:
        json.dump({"digests": T.digests(mods), "refusals": T.refusals(mods)}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", T.FIXTURE)
