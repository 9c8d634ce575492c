"""Stage-II throughput of the SMAL animal types: frames/s of a 4000-frame synthetic horse and dog sequence (40 markers, dropouts and
gaps), through StageIISolver as mosh_stageii drives it, in chain_mode 'auto' (chunked at this length) and 'sequential'.  Each mode is
timed after one untimed warm-up solve.  Prints one JSON line.

    python tools/animal_bench.py [--frames 4000] [--markers 40] [--reps 1]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=4000)
    ap.add_argument('--markers', type=int, default=40)
    ap.add_argument('--reps', type=int, default=1)
    a = ap.parse_args()
    from moshpp_amd import build, capi, synth
    from moshpp_amd.chmosh import StageIISolver
    from moshpp_amd.models import load_surface_model
    from moshpp_amd.prior import create_body_prior
    from oracle.stageii_oracle import stageii_weights_default
    capi.load()
    capi.require_device()
    res = {'tool': 'animal_bench', 'frames': a.frames, 'markers': a.markers, 'source_hash': build.source_hash()}
    for mt in ('animal_horse', 'animal_dog'):
        s = synth.make_sequence(mt, a.frames, a.markers, seed=21, body_only_markers=False)
        raw = {k: v for k, v in s['model'].items() if not k.startswith('_') and k != 'model_type'}
        sm = load_surface_model(raw)
        solver = StageIISolver(sm, s['betas'], s['markers_latent'], create_body_prior(mt, s['animal_prior']), stageii_weights_default(),
                               surface_model_type=mt, num_betas=s['num_betas'])
        obs, vis = np.nan_to_num(s['markers']), ~np.isnan(s['markers']).any(-1)
        for mode in ('auto', 'sequential'):
            solver.solve(obs, vis, chain_mode=mode)
            best = None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out = solver.solve(obs, vis, chain_mode=mode)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            res[f'{mt}_{mode}_fps'] = round(a.frames / best, 1)
            res[f'{mt}_{mode}_ran'] = out['chain_mode']
            res[f'{mt}_{mode}_failed_frames'] = int(np.sum(out['status'] < 0))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
