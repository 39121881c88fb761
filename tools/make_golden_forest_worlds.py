"""Fixture: the first four worlds of the reference's forest set and the mission that goes with the first -- the protocol of
launch/test_all_forest.launch, which pairs mission k of missions/forest10 with world k of world/forest (Mission::loadMission,
src/mission.cpp:82-92): worlds of ONE shape (same box, same resolution) with different pillars.  The rows of world/forest/forest1.csv ...
forest4.csv (centre x,y,z, size x,y,z; 40 boxes each, read by MapManager::updateOctreeFromCSV), the world box of the mission file and the
agents of missions/forest10/forest10_1.json.  Data only; run in the build container.

    python tools/make_golden_forest_worlds.py  ->  tests/golden/forest_worlds.json
"""
import csv
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
N_WORLDS = 4


def main():
    worlds = []
    for k in range(1, N_WORLDS + 1):
        rows = csv.reader(open(os.path.join(REF, "world/forest/forest%d.csv" % k)))
        worlds.append([[float(v) for v in row[:6]] for row in rows if len(row) >= 6])
    m = json.load(open(os.path.join(REF, "missions/forest10/forest10_1.json")))
    dim = m["world"][0]["dimension"]
    out = {"source": "reference world/forest/forest1.csv .. forest4.csv, missions/forest10/forest10_1.json; launch/test_all_forest.launch "
                     "(mission k over world k); launch/simulation.launch:56-60 (2-D, z = 1 as the mission file has it, resolution 0.1)",
           "worlds": worlds, "world_min": dim[:3], "world_max": dim[3:], "resolution": 0.1, "max_dist": 1.0, "z_2d": 1.0, "radius": 0.15,
           "starts": [a["start"][:3] for a in m["agents"]], "goals": [a["goal"][:3] for a in m["agents"]]}
    with open(os.path.join(ROOT, "tests", "golden", "forest_worlds.json"), "w") as f:
        json.dump(out, f)
    print([len(w) for w in worlds], "boxes,", len(out["starts"]), "agents")


if __name__ == "__main__":
    main()
