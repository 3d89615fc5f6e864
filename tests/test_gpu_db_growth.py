"""The database's arrays through every regrow and every ingest path: two engines per grid, A with initial_capacity=8 (grows five times
on the way to 150 keyframes) and B with initial_capacity=256 (never grows), receive the same 150 keyframes in the same order through
every append path in turn, with a query staged BEFORE the first keyframe so that its row moves through every regrow of A.  Whatever
reads the nine per-keyframe arrays must then agree on A and B bit for bit; A's distances must also be the CPU checker's."""
import numpy as np
import pytest

import oracle_binding as ob
from scl_slam_amd import ScanContextEngine
from scl_slam_amd.synth import synth_descriptors, synth_scan

pytestmark = pytest.mark.gpu

N = 150
EXCLUDE = 10          # num_exclude_recent: small, so that the streaming ingests' detections have something to search


_clouds = []


def scans():
    """the 150 clouds of about 2 000 points, made once for the three grids"""
    if not _clouds:
        _clouds.extend(synth_scan(1900 + 13 * (i % 16), seed=500 + i) for i in range(N))
    return _clouds


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(a.view(u), b.view(u))


def fill(eng, clouds, wire, staged):
    """the 150 keyframes through every ingest path in turn; returns what the two streaming ingests returned"""
    eng.stage_query(staged)                                                   # before the first keyframe
    at = 0
    for _ in range(3):
        eng.make_and_save(clouds[at], robot=0, index=at); at += 1
    for _ in range(3):
        eng.make_and_save_filtered(clouds[at], 0.4, robot=0, index=at); at += 1
    eng.save_bulk(wire[at:at + 7]); at += 7
    # 16 clouds laid out one behind the other in ONE pinned allocation (the merged copy), then 5 from arrays of their own
    counts = [c.shape[0] for c in clouds[at:at + 16]]
    arena = eng.host_alloc((sum(counts), 8))
    views, o = [], 0
    for c in clouds[at:at + 16]:
        arena[o:o + c.shape[0]] = c
        views.append(arena[o:o + c.shape[0]]); o += c.shape[0]
    eng.make_and_save_many(views, want_values=False); at += 16
    eng.host_free(arena)
    apart = []                                                                # (every other one 4 bytes off the allocator's 16: never one copy)
    for i, c in enumerate(clouds[at:at + 5]):
        v = np.empty(c.size + 4, np.float32)[i % 2:i % 2 + c.size].reshape(c.shape)
        v[:] = c
        apart.append(v)
    eng.make_and_save_many(apart); at += 5
    from_points = eng.stream_from_points(clouds[at:at + 20]); at += 20
    for i in range(33):
        eng.keyframe_put(0, i, clouds[at + i])
    from_store = eng.stream_from_store(0, 0, 33); at += 33
    eng.save_bulk(wire[at:N])
    assert eng.get_size() == N
    return from_points, from_store


@pytest.mark.parametrize("R,S", [(20, 60), (64, 120), (80, 180)])   # no screening, screened, wide
def test_growth_through_every_ingest_path_keeps_every_array(R, S):
    clouds = scans()
    a = ScanContextEngine(num_ring=R, num_sector=S, num_exclude_recent=EXCLUDE, initial_capacity=8)
    b = ScanContextEngine(num_ring=R, num_sector=S, num_exclude_recent=EXCLUDE, initial_capacity=256)
    try:
        wire = np.stack([a.make_descriptor(c) for c in clouds])                # what save_bulk appends (nothing is stored by this)
        staged = synth_descriptors(1, R, S, seed=77)[0]
        ra, rb = fill(a, clouds, wire, staged), fill(b, clouds, wire, staged)
        for xa, xb in zip(ra[0] + ra[1], rb[0] + rb[1]):                        # the loop results of the two streaming ingests
            assert same_bits(xa, xb)
        descs = a.get_descriptors(0, N)
        assert same_bits(descs, b.get_descriptors(0, N))
        for s in range(N):
            assert same_bits(a.get_ringkey(s), b.get_ringkey(s)), s
            assert same_bits(a.get_sectorkey(s), b.get_sectorkey(s)), s
        qs = np.arange(N - 40, N, dtype=np.int32)
        calls = [
            lambda e: e.sc_distance_batch(-1, n=N),                           # the staged query
            lambda e: e.sc_distance_batch(N - 1, n=N),
            lambda e: e.ringkey_topk(N - 1, 0, N - EXCLUDE, 10)[:2],
            lambda e: e.topk_with_distance(N - 1, 0, N - EXCLUDE, 10)[:4],
            lambda e: [np.asarray(v) for v in e.detect_full(N - 1)],
            lambda e: e.detect_full_stream(qs, 0, qs - EXCLUDE, 16, 2),
            lambda e: e.sc_distance_matrix([N - 1, 100, 50, 7, -1], 0, N),
            lambda e: e.sc_search([N - 1, 120, 90, 60, 30], 3),
        ]
        for i, call in enumerate(calls):
            for xa, xb in zip(call(a), call(b)):
                assert same_bits(xa, xb), i
        # ... and the grown database's distances are the checker's
        db = ob.OracleDB(ob.make_config(R=R, S=S, exclude_recent=EXCLUDE)); db.save_bulk(descs)
        d_gpu, s_gpu = a.sc_distance_batch(N - 1, n=N)
        d_cpu, s_cpu = db.distance_batch(N - 1, n=N, fast=True)
        assert np.array_equal(s_gpu, s_cpu)
        assert np.array_equal(d_gpu.view(np.uint64), d_cpu.view(np.uint64)), f"max |diff| = {np.nanmax(np.abs(d_gpu - d_cpu))}"
    finally:
        a.close(); b.close()
