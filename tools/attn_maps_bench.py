"""Beam search of the R2Gen decoder with and without attention maps, timed at the BASELINE config 5 decode geometry: 32 studies x 144
encoder tokens (384 x 384), beam 4, max_seq_len 100, procedural weights, the encoder states fed directly (no trunk runs).  Per route two
warm-up searches, then --runs timed ones: the per-token step time from the HIP events of the token loop (decode.stats['step_events'])
and the kernel launches of one captured step.  Then the cross-attention launch alone at the same geometry (128 rows x 8 heads, four rows
per K / V row): evk_decode_attention and evk_decode_attention_maps, each as the median of --launches event pairs around one launch and as
the mean of the same launches issued back to back.

The maps legs are skipped where the tree has no return_attention (--plain-only forces that), so the same file measures an earlier commit.

    python tools/attn_maps_bench.py [--studies 32] [--beam 4] [--max-seq-len 100] [--tokens 144] [--runs 3] [--plain-only]"""
import argparse
import ctypes as C
import inspect
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed_searches(decode, dec, args, runs, **kw):
    out = []
    for i in range(2 + runs):
        decode.stats.pop('step_events', None)
        decode.beam_search(dec, None, None, args, **kw)
        torch.cuda.synchronize()
        ev0, ev1, n = decode.stats['step_events']
        if i >= 2:
            out.append(round(ev0.elapsed_time(ev1) / n * 1e3, 2))
    return dict(step_us=out, step_launches=decode.stats.get('step_launches'), graph=bool(decode.stats.get('graph')))


def timed_launch(fn, n):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    single = statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return dict(single_us=round(single, 2), back_to_back_us=round(a.elapsed_time(b) / n * 1e3, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--studies', type=int, default=32)
    ap.add_argument('--beam', type=int, default=4)
    ap.add_argument('--max-seq-len', type=int, default=100)
    ap.add_argument('--tokens', type=int, default=144)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--plain-only', action='store_true')
    a = ap.parse_args()
    from evoke_amd import decode, hip as H, ops
    from evoke_amd.config import ARGS
    from evoke_amd.layers import EncoderDecoder
    from evoke_amd.tokenizer import load_tokenizer
    from oracle import spec as S
    V = 1444
    tok = load_tokenizer(os.path.join(REPO, 'tests', 'golden', 'iu_xray_wordlevel_uncased_tokenizer.json'))
    args = dict(ARGS, beam_size=a.beam, max_seq_len=a.max_seq_len)
    dec = EncoderDecoder(args, tok)
    sd = {k[len('text_decoder.'):]: v for k, v in S.procedural_state(S.finetune_spec(V)).items() if k.startswith('text_decoder.')}
    dec.load_state_dict(sd)
    dec = dec.cuda().eval()
    ops.set_dropout_enabled(False)
    enc = (S.det((a.studies, a.tokens, 512), a=.013, b=.007, c=.3) * 0.5).to(ops.BF16).cuda()
    dec.encode = lambda states, mask: (enc, None)
    has_maps = not a.plain_only and 'return_attention' in inspect.signature(decode.beam_search).parameters
    rec = dict(studies=a.studies, beam=a.beam, max_seq_len=a.max_seq_len, tokens=a.tokens, plain=timed_searches(decode, dec, args, a.runs))
    if has_maps:
        rec['maps'] = timed_searches(decode, dec, args, a.runs, return_attention=True)
        rec['plain_again'] = timed_searches(decode, dec, args, a.runs)
    # the cross-attention launch alone
    R, heads, S_ = a.studies * a.beam, 8, a.tokens
    g = torch.Generator().manual_seed(0)
    q = (torch.rand(R, heads * 64, generator=g) - 0.5).to(ops.BF16).cuda()
    k = (torch.rand(a.studies, S_, heads * 64, generator=g) - 0.5).to(ops.BF16).cuda()
    v = (torch.rand(a.studies, S_, heads * 64, generator=g) - 0.5).to(ops.BF16).cuda()
    out = torch.empty_like(q)
    scale = C.c_float(0.125)
    rec['launch_plain'] = timed_launch(lambda: H.check(H.lib.evk_decode_attention(H.ptr(q), H.ptr(k), H.ptr(v), None, H.ptr(out), R, S_, heads, 64,
                                                                                 a.beam, scale, H.stream())), a.launches)
    if has_maps:
        maps = torch.empty(4, R, 3 * S_, dtype=torch.float32, device='cuda')
        pos = torch.tensor([1], dtype=torch.long, device='cuda')
        rec['launch_maps'] = timed_launch(lambda: H.check(H.lib.evk_decode_attention_maps(H.ptr(q), H.ptr(k), H.ptr(v), None, H.ptr(out), H.ptr(maps),
                                                                                         3 * S_, H.ptr(pos), maps.stride(0), R, S_, heads, 64, a.beam,
                                                                                         scale, H.stream())), a.launches)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
