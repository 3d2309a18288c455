"""The two ends of the backward's dgrad chain in a kernel trace of the training step.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python bench.py --gpus 1 --steps 20 --warmup 5
    python tools/backward_ends_timeline.py DIR/**/NAME_kernel_trace.csv [--label BEFORE]

Reads the trace CSV (one row per dispatch: kernel name, queue and stream ids, start and end in ns) and prints, for the LAST step of the run,
  TOP     start of cls_tail_bwd_kernel            -> start of the first attn_bwd_kernel<false>
  BOTTOM  end of the last attn_bwd_kernel<false>  -> start of sq_norm_clip_kernel
with every kernel that runs inside the segment (queue, stream, start and end relative to the segment's start, duration), the segment's
length, and the per-kernel averages over all steps of the kernels that appear in either segment (calls per step, mean us)."""
import argparse
import collections
import csv
import re


def short(name):
    name = name.replace('(anonymous namespace)::', '').replace('void ', '')
    m = re.match(r'_ZN12_GLOBAL__N_1\d+([A-Za-z_0-9]+?)I', name)          # a mangled template instance
    if m:
        return m.group(1)
    return re.sub(r'\(.*', '', name)


def load(path):
    rows = []
    with open(path, newline='') as f:
        for r in csv.DictReader(f):
            rows.append({'name': short(r['Kernel_Name']), 'q': r.get('Queue_Id', '?'), 's': r.get('Stream_Id', '?'),
                         't0': int(r['Start_Timestamp']), 't1': int(r['End_Timestamp'])})
    rows.sort(key=lambda r: r['t0'])
    return rows


def segment(rows, t_from, t_to):
    """kernels that overlap [t_from, t_to]"""
    return [r for r in rows if r['t1'] > t_from and r['t0'] < t_to]


def show(title, rows, t_from, t_to):
    inside = [r['t1'] for r in segment(rows, t_from, t_to) if r['t0'] >= t_from]
    # (the segment's end is a launch of the optimizer: with the host behind, e.g. under the profiler, the device work ends well before it)
    print('%s: %.1f us; the last kernel started inside it ends at %.1f us' % (title, (t_to - t_from) / 1e3,
                                                                             (max(inside) - t_from) / 1e3 if inside else 0.0))
    print('  %-5s %-6s %9s %9s %8s  %s' % ('queue', 'stream', 'start_us', 'end_us', 'dur_us', 'kernel'))
    for r in segment(rows, t_from, t_to):
        print('  %-5s %-6s %9.1f %9.1f %8.1f  %s' % (r['q'], r['s'], (r['t0'] - t_from) / 1e3, (r['t1'] - t_from) / 1e3,
                                                     (r['t1'] - r['t0']) / 1e3, r['name']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('trace')
    ap.add_argument('--label', default='')
    a = ap.parse_args()
    rows = load(a.trace)
    is_attn = lambda r: r['name'].startswith('attn_bwd_kernel<false>')
    tails = [i for i, r in enumerate(rows) if r['name'].startswith('cls_tail_bwd_kernel')]
    clips = [i for i, r in enumerate(rows) if r['name'].startswith('sq_norm_clip_kernel')]
    if not tails or not clips or clips[-1] < tails[-1]:
        raise SystemExit('no complete training step in the trace (cls_tail_bwd_kernel ... sq_norm_clip_kernel)')
    i0, i1 = tails[-1], clips[-1]
    attn = [r for r in rows[i0:i1] if is_attn(r)]
    if not attn:
        raise SystemExit('no attn_bwd_kernel<false> between the last cls_tail_bwd_kernel and sq_norm_clip_kernel')
    if a.label:
        print('==== %s ====' % a.label)
    print('last of %d steps in %s' % (len(tails), a.trace.split('/')[-1]))
    top = (rows[i0]['t0'], attn[0]['t0'])
    bottom = (max(r['t1'] for r in attn), rows[i1]['t0'])
    show('TOP (cls_tail_bwd start -> first attn_bwd<false> start)', rows, *top)
    show('BOTTOM (last attn_bwd<false> end -> sq_norm_clip start)', rows, *bottom)
    names = {r['name'] for seg in (top, bottom) for r in segment(rows, *seg)}
    names |= {r['name'] for r in rows if r['name'].startswith('mlp_fused_kernel<1,')}       # every form of the backward's MLP launch
    agg = collections.defaultdict(list)
    for r in rows[tails[0]:]:
        if r['name'] in names:
            agg[r['name']].append((r['t1'] - r['t0']) / 1e3)
    steps = len(tails)
    print('per-kernel averages over the %d steps (kernels of either segment, and the MLP launches of the backward):' % steps)
    print('  %-12s %9s  %s' % ('calls/step', 'mean_us', 'kernel'))
    for n in sorted(agg, key=lambda n: -sum(agg[n])):
        print('  %-12.2f %9.1f  %s' % (len(agg[n]) / steps, sum(agg[n]) / len(agg[n]), n))


if __name__ == '__main__':
    main()
