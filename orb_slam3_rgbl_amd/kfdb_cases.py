"""Generators for KeyFrameDatabase cases: a database with loop structure, queries, covisibility lists and mutation scripts.

Key frames lie along a trajectory.  Every place p of the trajectory sees a window of a long random "scene" of vocabulary
words, so neighbouring key frames share most of their words; the last stretch of the trajectory drives through the first
places again (a loop), and the key frames are spread over several maps.  BowVectors are what DBoW2's transform produces:
ascending distinct word ids and positive values that are L1-normalised in double.
"""
import numpy as np


def _bow(rng, scene, place, stride, window, n_words, n_vocab, noise):
    """One BowVector seen from `place`."""
    lo = place * stride
    pool = np.unique(scene[lo:lo + window])
    n_scene = min(len(pool), int(round(n_words * (1.0 - noise))))
    ids = rng.choice(pool, n_scene, replace=False)
    extra = rng.integers(0, n_vocab, n_words - n_scene)
    ids = np.unique(np.concatenate([ids, extra])).astype(np.uint32)
    val = rng.uniform(0.5, 9.0, len(ids)) * rng.integers(1, 4, len(ids))     # idf weight times term count
    val = val / val.sum()                                                      # L1 normalisation (BowVector::normalize)
    return ids, val.astype(np.float64)


def make_database(n_kf=200, n_words=120, n_vocab=20000, seed=0, n_maps=2, loop_fraction=0.2, noise=0.15):
    """dict(n_vocab, entries=[dict(kf_id, map_id, place, word_id, word_val)], scene, stride, window, n_words, noise, seed)."""
    rng = np.random.default_rng(0xDB0 + seed)
    stride = max(1, n_words // 6)
    window = n_words * 2
    n_loop = int(n_kf * loop_fraction)
    n_places = max(1, n_kf - n_loop)
    scene = rng.integers(0, n_vocab, n_places * stride + window)
    entries = []
    for i in range(n_kf):
        place = i if i < n_places else (i - n_places) % n_places               # the loop: back at the start
        ids, val = _bow(rng, scene, place, stride, window, n_words, n_vocab, noise)
        # a new map every n_kf / n_maps key frames; the revisiting stretch lies in the last one
        entries.append(dict(kf_id=1000 + 7 * i, map_id=min(n_maps - 1, i * n_maps // max(n_kf, 1)), place=place, word_id=ids, word_val=val))
    return dict(n_vocab=n_vocab, entries=entries, scene=scene, stride=stride, window=window, n_words=n_words, noise=noise, seed=seed,
                n_places=n_places)


def make_query(db, place, seed=0, n_words=None):
    """A frame's BowVector seen from `place` of the database's trajectory."""
    rng = np.random.default_rng(0x9E7 + 31 * seed + place)
    return _bow(rng, db["scene"], place % db["n_places"], db["stride"], db["window"], n_words or db["n_words"], db["n_vocab"], db["noise"])


def covisibility(db, n_best=10, seed=0):
    """{kf_id: covisible key frames, best first}: trajectory neighbours, then the key frames that see the same place."""
    ent = db["entries"]
    rng = np.random.default_rng(0xC0F + seed)
    out = {}
    for i, e in enumerate(ent):
        near = [j for d in range(1, 5) for j in (i - d, i + d) if 0 <= j < len(ent)]
        same = [j for j, o in enumerate(ent) if j != i and abs(o["place"] - e["place"]) <= 1 and j not in near]
        order = near + same
        keep = int(rng.integers(0, n_best + 4))
        out[e["kf_id"]] = [ent[j]["kf_id"] for j in order[:keep]]
    return out


def connected(db, i, reach=6):
    """GetConnectedKeyFrames() of entry i: its trajectory neighbours."""
    ent = db["entries"]
    return {ent[j]["kf_id"] for j in range(max(0, i - reach), min(len(ent), i + reach + 1)) if j != i}


def mutation_script(db, seed=0, n_ops=60):
    """A sequence of ("add", i) / ("erase", i) / ("clear_map", m) / ("query", place) over the database's entries: everything is
    added first, then key frames are erased, some added again (they go to the end of the order), one map is cleared."""
    rng = np.random.default_rng(0x5C1 + seed)
    n = len(db["entries"])
    ops = [("add", i) for i in range(n)]
    inside = set(range(n))
    n_maps = 1 + max(e["map_id"] for e in db["entries"])
    cleared = False
    for k in range(n_ops):
        r = rng.random()
        if r < 0.35 and inside:
            i = int(rng.choice(sorted(inside)))
            ops.append(("erase", i))
            inside.discard(i)
        elif r < 0.6 and len(inside) < n:
            i = int(rng.choice(sorted(set(range(n)) - inside)))
            ops.append(("add", i))
            inside.add(i)
        elif r < 0.65 and not cleared and n_maps > 1:
            m = int(rng.integers(0, n_maps))
            ops.append(("clear_map", m))
            inside -= {i for i in inside if db["entries"][i]["map_id"] == m}
            cleared = True
        else:
            ops.append(("query", int(rng.integers(0, db["n_places"]))))
    ops.append(("query", 0))
    return ops
