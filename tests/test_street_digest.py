"""CPU: gfxh_scene_make_street builds, byte for byte, the scenes whose digests tests/golden/street_digest.json holds -- the small
streets of the tests and the street bench.py measures, plain, textured and cluttered.  The GPU parity tests compare the GPU with the
oracle on whatever street they are given; this test is what notices that the street itself changed (and with it every number
measured on it).  tests/golden/make_street_digest.py wrote the file and says what the digest covers."""
import json

import pytest

from tests.golden import make_street_digest as D

with open(D.OUT) as _f:
    GOLDEN = json.load(_f)


def test_the_digest_file_names_the_scenes():
    assert sorted(GOLDEN) == sorted(D.SCENES) and len(GOLDEN) == 9
    assert len(set(GOLDEN.values())) == 9                   # textured, cluttered and scale each change the scene


@pytest.mark.parametrize("name", sorted(D.SCENES))
def test_the_street_is_the_committed_one(built_lib, name):
    assert D.scene_digest(name) == GOLDEN[name]
