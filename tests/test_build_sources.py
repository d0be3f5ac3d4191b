"""build.SOURCES is the link line: a translation unit of csrc/ that it does not name is silently left out of the library (its launch
functions then fail to resolve only when the library is loaded), and one named twice is linked twice."""
import os

from lfr_amd import build


def test_sources_name_every_unit_once():
    on_disk = sorted(f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp")))
    assert on_disk, "no sources found under %s" % build.CSRC
    assert sorted(build.SOURCES) == on_disk          # (a directory listing has no duplicates: every unit once)
