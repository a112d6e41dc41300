"""The figures of profiles/live_notes.md section 2 (DESIGN SPEC 3.12), one JSON line per mode; driven by tools/live_ab.sh.

    python tools/live_measure.py tuner    SondeTuner.process, every VFO of sonde_tuner_create active (SONDE_MI355_LIB picks the library: A/B)
    python tools/live_measure.py idle     8 active slots alone against 8 active slots beside 64 idle ones
    python tools/live_measure.py live     LiveReceiver against WidebandReceiver(track=True), 4 sondes; the scanner's and the probe slots' parts
"""
import sys, os, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from sdrpp_radiosonde_amd import _lib, synth
from sdrpp_radiosonde_amd.tuner import SondeTuner, WidebandReceiver
DEV = "cuda:0"

def ev_ms(fn, reps, warm=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps

mode = sys.argv[1]
if mode == "tuner":          # the unchanged case: sonde_tuner_create, every VFO active; 10 MS/s, 0.128 s blocks, 8 VFOs of three bandwidths
    fs, n = 10_000_000, 1_280_000
    blk = torch.randn((n, 2), device=DEV)
    vf = [(-4_000_000 + 1_000_003 * k, [10_000, 20_000, 40_000][k % 3]) for k in range(8)]
    tu = SondeTuner(fs, 48_000, vf, n)
    out = torch.empty((8, tu.out_samples(n), 2), device=DEV)
    ms = [ev_ms(lambda: tu.process(blk, out=out), 40) for _ in range(3)]
    print(json.dumps({"mode": mode, "lib": os.environ.get("SONDE_MI355_LIB", "tree"), "ms_per_process": ms}))
elif mode == "idle":
    fs, n = 10_000_000, 1_280_000
    blk = torch.randn((n, 2), device=DEV)
    vf = [(-4_000_000 + 1_000_003 * k, [10_000, 20_000, 40_000][k % 3]) for k in range(8)]
    res = {}
    for n_slots in (8, 72):
        tu = SondeTuner.slots(fs, 48_000, n_slots, [10_000, 20_000, 40_000], n)
        for k, (f, b) in enumerate(vf): tu.slot_set(k, f, b)
        out = torch.empty((n_slots, tu.out_samples(n), 2), device=DEV)
        res[f"{n_slots}_slots_8_active"] = [ev_ms(lambda: tu.process(blk, out=out), 40) for _ in range(3)]
        tu.close()
    print(json.dumps({"mode": mode, "ms_per_process": res}))
elif mode == "live":
    from sdrpp_radiosonde_amd.live import LiveReceiver
    from sdrpp_radiosonde_amd.scan import SondeScanner
    from sdrpp_radiosonde_amd.detect import SondeDetector
    FS, G = 1_000_000, 128_000
    sondes = [(-400_000, 0), (-250_000, 1), (250_000, 3), (100_000, 0)]
    N = 40 * G
    iq, _, _ = synth.make_wideband_scene(sondes, N, fs=FS, seed=77, device=DEV)
    iq = iq.contiguous()
    blocks = [iq[a:a + G] for a in range(0, N, G)]
    def run(rx):
        # stream time of the submits of the last 24 blocks (the first 16 warm up and let the loops settle), host bookkeeping between them included
        for b in blocks[:16]: rx.submit(b)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); dev = 0.0
        for b in blocks[16:]:
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); rx.submit(b); e.record(); e.synchronize(); dev += a.elapsed_time(e)
        return dev / 24, (time.perf_counter() - t0) * 1e3 / 24
    out = {}
    for rep in range(3):
        wb = WidebandReceiver(FS, sondes, chain="iq48", track=True)
        out.setdefault("wideband_track_4vfos", []).append(run(wb)); wb.close()
        lv = LiveReceiver(FS, {0: 2, 1: 1, 3: 1}, probes=4, initial=sondes, scan_seconds=1.024, probe_seconds=2.048)
        out.setdefault("live_4of4_decode_0of4_probes", []).append(run(lv)); lv.close()
        lv = LiveReceiver(FS, {0: 2, 1: 1, 3: 1}, probes=4, initial=sondes, scan_seconds=1e9, probe_seconds=2.048)
        lv.scanner.submit = lambda *a, **k: None
        out.setdefault("live_without_scanner", []).append(run(lv)); lv.close()
    # the parts alone, kernels only (no host work between them)
    sc = SondeScanner(FS, G)
    out["scanner_submit_alone_ms"] = [ev_ms(lambda: sc.submit(blocks[3]), 50) for _ in range(3)]
    for act in (0, 1, 4):
        tu = SondeTuner.slots(FS, 48_000, 8, [10_000, 15_000, 40_000], G)
        for k, (f, t) in enumerate(sondes): tu.slot_set(k, f, [10_000, 15_000, 40_000, 10_000][k])
        for p in range(act): tu.slot_set(4 + p, 400_000 - 50_000 * p, 40_000)
        rows = torch.empty((8, 6144, 2), device=DEV)
        det = SondeDetector(4, 6144)
        def step():
            tu.process(blocks[3], out=rows); det.submit(rows[4:])
        out[f"tuner8_plus_detector4_{act}_probes_active_ms"] = [ev_ms(step, 50) for _ in range(3)]
        tu.close(); det.close()
    print(json.dumps({"mode": mode, "ms_per_submit(stream, wall)": out}))
