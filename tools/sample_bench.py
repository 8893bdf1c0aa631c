"""Greedy sampling decode (decode.sample, csrc/sample.hip) against beam search with one beam (decode.beam_search, csrc/beam.hip) on the same
encoder states: R = 64 studies of two 384^2 views (built as bench.py --workload decode builds them), max_seq_len 100.  Per route: positions
per second of whole calls (wall clock, device synchronised), the per-token step time (HIP events around the replays) and the kernel
launches of one captured token step.
usage: python tools/sample_bench.py [runs=3] [batch=64] [res=384] [method=greedy]"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import make_args, synth_batch  # noqa: E402
from evoke_amd import decode as DEC  # noqa: E402
from evoke_amd.config import load_default_tokenizer  # noqa: E402
from evoke_amd.model_pretrain_finetune import FineTune  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
res = int(sys.argv[3]) if len(sys.argv) > 3 else 384
method = sys.argv[4] if len(sys.argv) > 4 else 'greedy'
L, dev = 100, torch.device('cuda')

torch.manual_seed(9233)
model = FineTune(make_args('test'), load_default_tokenizer(), 'mimic_cxr').to(dev)
model.train()
wb = synth_batch('finetune', min(B, 16), 2, res, L, 30, dev, 3000)
with torch.no_grad():
    for _ in range(40):                           # running statistics of a network that has seen data (fresh ones overflow fp16 in eval mode)
        model.visual_extractor(wb['images'])
model.eval()
b = synth_batch('finetune', B, 2, res, L, 30, dev, 2000)
with torch.no_grad():
    x, enc_mask = model.encoder_states(b['images'], b['pids'], B, b['inc'], b['inc_masks'])
torch.cuda.synchronize()

routes = {
    'sample': lambda: DEC.sample(model.text_decoder, x, enc_mask, dict(model.args, beam_size=1, max_seq_len=L, sample_method=method))[0],
    'beam_search_beam1': lambda: DEC.beam_search(model.text_decoder, x, enc_mask, dict(model.args, beam_size=1, max_seq_len=L)),
}
out = {'rows': B, 'max_seq_len': L, 'res': res, 'sample_method': method, 'runs': runs}
for name, fn in routes.items():
    for _ in range(2):                            # first call: session build, warm-up steps, capture
        fn()
    torch.cuda.synchronize()
    rate, step_us = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        rate.append(B * L / (time.perf_counter() - t0))
        ev0, ev1, cnt = DEC.stats['step_events']
        step_us.append(1e3 * ev0.elapsed_time(ev1) / max(cnt, 1))
    out[name] = {'positions_per_s': [round(v) for v in rate], 'step_us': [round(v, 1) for v in step_us],
                 'launches_per_token_step': DEC.stats.get('step_launches')}
print(json.dumps(out))
