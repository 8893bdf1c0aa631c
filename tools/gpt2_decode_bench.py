"""Beam search of the distilgpt2 decoder backend, timed: 32 studies x 50 encoder positions, the decoder sizes of the EVOKE YAML files
(3 layers x 2048 x 8 heads), beam 3, max_seq_len 100, procedural weights.  Two warm-up calls, then three timed runs of
DistilGPT2TextDecoderModel.generate(); per run: wall seconds, tokens/s (studies x generated positions of the returned ids / seconds), and --
where the search runs as a device session -- the per-token step time from the HIP events of the token loop and the launches of one
captured step.  Uses only the public generate(), so the same file measures a commit from before the device session.

--do-sample / --top-k / --top-p / --repetition-penalty time the sampling route (gpt2_decode._GPT2SampleSession, --beam 1) instead; the
uniform numbers are drawn once, outside the timed calls, so that every run draws the same reports.

--num-beams / --no-repeat-ngram-size / --min-length / --length-penalty / --early-stopping time the beam search with options
(gpt2_decode._GPT2BeamOptionsSession; --repetition-penalty joins them once one of them is given).  Without them the call carries no new
keyword, so the same file still measures a commit from before them.

    python tools/gpt2_decode_bench.py [--studies 32] [--beam 3] [--max-seq-len 100] [--runs 3]
                                      [--do-sample] [--top-k K] [--top-p P] [--repetition-penalty RP]
                                      [--num-beams N] [--no-repeat-ngram-size G] [--min-length M] [--length-penalty LP] [--early-stopping]"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--studies', type=int, default=32)
    ap.add_argument('--beam', type=int, default=3)
    ap.add_argument('--max-seq-len', type=int, default=100)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--do-sample', action='store_true')
    ap.add_argument('--top-k', type=int, default=0)
    ap.add_argument('--top-p', type=float, default=1.0)
    ap.add_argument('--repetition-penalty', type=float, default=1.0)
    ap.add_argument('--num-beams', type=int, default=None)
    ap.add_argument('--no-repeat-ngram-size', type=int, default=0)
    ap.add_argument('--min-length', type=int, default=0)
    ap.add_argument('--length-penalty', type=float, default=None)
    ap.add_argument('--early-stopping', action='store_true')
    a = ap.parse_args()
    from evoke_amd import decode, ops
    from evoke_amd.config import ARGS
    from evoke_amd.gpt2 import DistilGPT2TextDecoderModel
    from evoke_amd.tokenizer import load_tokenizer
    from oracle import gpt2 as G, spec as S
    V, d, layers, heads = 1444, 2048, 3, 8
    tok = load_tokenizer(os.path.join(REPO, 'tests', 'golden', 'iu_xray_wordlevel_uncased_tokenizer.json'))
    args = dict(ARGS, decoder_hidden_size=d, decoder_num_hidden_layers=layers, decoder_num_attention_heads=heads, beam_size=a.beam,
                max_seq_len=a.max_seq_len)
    dec = DistilGPT2TextDecoderModel(args, tok)
    sd = {k[len('text_decoder.'):]: v for k, v in S.procedural_state(G.gpt2_spec(V, d, layers)).items()}
    sd['decoder.encoder_decoder.decoder.lm_head.weight'] = sd['decoder.encoder_decoder.decoder.transformer.wte.weight']
    dec.load_state_dict(sd)
    dec = dec.cuda().eval()
    ops.set_dropout_enabled(False)
    enc = (S.det((a.studies, 50, d), a=.013, b=.007, c=.3) * 0.5).to(ops.BF16).cuda()
    kw = {}
    if a.do_sample or a.repetition_penalty != 1.0:                       # (no keyword at all otherwise: the call a commit without them accepts)
        kw = dict(do_sample=a.do_sample, top_k=a.top_k, top_p=a.top_p, repetition_penalty=a.repetition_penalty)
        if a.do_sample:
            kw['uniforms'] = torch.rand(a.studies, a.max_seq_len, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    if a.num_beams is not None or a.no_repeat_ngram_size or a.min_length or a.length_penalty is not None or a.early_stopping:
        # the beam search with options: the width is given explicitly, which is what takes generate() to that route
        kw = dict(num_beams=a.num_beams if a.num_beams is not None else a.beam, repetition_penalty=a.repetition_penalty,
                  no_repeat_ngram_size=a.no_repeat_ngram_size, min_length=a.min_length, early_stopping=a.early_stopping,
                  length_penalty=a.length_penalty if a.length_penalty is not None else 1.0)
    runs = []
    for i in range(2 + a.runs):
        decode.stats.pop('step_events', None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq = dec.generate(enc, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rec = dict(seconds=round(dt, 4), width=int(seq.shape[1]), tokens_per_s=round(a.studies * (seq.shape[1] - 1) / dt, 1))
        ev = decode.stats.get('step_events')
        if ev is not None and ev[2] > 0:
            rec['step_ms'] = round(ev[0].elapsed_time(ev[1]) / ev[2], 4)
            rec['step_launches'] = decode.stats.get('step_launches')
            rec['steps_issued'] = decode.stats.get('gpt2_steps_issued')
        if i >= 2:
            runs.append(rec)
    print(json.dumps(dict(studies=a.studies, beam=a.beam, max_seq_len=a.max_seq_len, route=decode.stats.get('gpt2_route', 'beam'),
                          options={k: v for k, v in kw.items() if k != 'uniforms'}, device_session=bool(getattr(dec, 'session_available', lambda *_: False)(50)),
                          runs=runs)))


if __name__ == '__main__':
    main()
