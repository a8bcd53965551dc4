"""Summarise DL_FS_STAMPS output: per launch, distribution of workgroup start times and per-phase durations (shader-clock ticks -> us at 2.4 GHz)."""
import sys
import numpy as np
blocks, cur = [], []
for line in open(sys.argv[1]):
    if line.startswith('#'):
        if cur: blocks.append(np.array(cur, dtype='f8')); cur = []
    else:
        cur.append([float(v) for v in line.split()])
GHZ = 2.4
for ib, a in enumerate(blocks):
    t0 = a[:, 0].min()
    rel = (a - t0) / GHZ / 1e3
    names = ['start', 'phase01', 'convolution', 'coefficients', 'projection', 'store']
    print('launch %d: %d workgroups' % (ib, len(a)))
    print('  workgroup start : min %.2f median %.2f p90 %.2f max %.2f us' % (rel[:, 0].min(), np.median(rel[:, 0]), np.percentile(rel[:, 0], 90), rel[:, 0].max()))
    for q in range(1, 6):
        d = rel[:, q] - rel[:, q - 1]
        print('  %-13s: median %.2f p90 %.2f max %.2f us' % (names[q], np.median(d), np.percentile(d, 90), d.max()))
    print('  workgroup life  : median %.2f max %.2f us; last exit at %.2f us' % (np.median(rel[:, 5] - rel[:, 0]), (rel[:, 5] - rel[:, 0]).max(), rel[:, 5].max()))
    # s_memtime differs between XCDs; slots 6 / 7 hold s_memrealtime (100 MHz, chip-wide) at entry / exit: the dispatch ramp
    if a.shape[1] >= 8:
        st = (a[:, 6] - a[:, 6].min()) * 0.01
        en = (a[:, 7] - a[:, 6].min()) * 0.01
        print('  chip-wide (100 MHz clock): workgroup starts: median %.2f p90 %.2f max %.2f us; exits: median %.2f max %.2f us' % (
            np.median(st), np.percentile(st, 90), st.max(), np.median(en), en.max()))
        print('  start time by workgroup id (every 64th): ' + ' '.join('%.1f' % v for v in st[::64]))
    if a.shape[1] >= 8:
        life = (a[:, 5] - a[:, 0]) / GHZ / 1e3
        q = len(life) // 4
        print('  workgroup life by id quartile: ' + ' '.join('%.2f' % np.median(life[i * q:(i + 1) * q]) for i in range(4)) + ' ; slowest ids: ' + ' '.join(str(i) for i in np.argsort(life)[-12:]))
    # slots 8 / 9: hardware ids (XCC id << 32 | HW_ID) of the waves of thread 0 (a spline wave) and of the mu wave: SIMD [5:4], CU [11:8], shader array / engine [15:12].
    # The three spline waves of a workgroup are heavy, its mu wave is light; with one wave per SIMD (checked on the two recorded waves) the heavy waves sit on the
    # SIMDs the mu wave does not.
    if a.shape[1] >= 10:
        import collections
        hw = a[:, 8:10].astype('u8')
        simd = ((hw >> np.uint64(4)) & np.uint64(3)).astype(int)
        cu = [(int(h >> np.uint64(32)) & 15, int(h >> np.uint64(8)) & 0xff) for h in hw[:, 0]]      # (XCC, shader engine / array / CU)
        same = sum(c == (int(h >> np.uint64(32)) & 15, int(h >> np.uint64(8)) & 0xff) for c, h in zip(cu, hw[:, 1]))
        print('  placement: %d workgroups on %d CUs (mu wave on the CU of wave 0: %d); (SIMD of wave 0, SIMD of the mu wave): %s' % (
            len(a), len(set(cu)), same, ' '.join('%d,%d:%d' % (k + (v,)) for k, v in sorted(collections.Counter(map(tuple, simd)).items()))))
        per_cu = collections.defaultdict(list)
        for w, c in enumerate(cu): per_cu[c].append(w)
        ncu = len(per_cu)
        light = collections.Counter()      # light (mu) waves per SIMD of a CU -> number of CUs
        gens = collections.Counter()       # id // (number of CUs) of the workgroups of a CU -> number of CUs
        for c, ws in per_cu.items():
            n = [0, 0, 0, 0]
            for w in ws: n[simd[w, 1]] += 1
            light[tuple(n)] += 1
            gens[tuple(sorted(w // ncu for w in ws))] += 1
        print('  light waves on SIMD 0 1 2 3 of a CU (heavy = workgroups of the CU - light) : CUs')
        for k, v in sorted(light.items(), key=lambda kv: -kv[1])[:8]: print('    %d %d %d %d : %d' % (k + (v,)))
        print('  workgroup id // %d of the workgroups of a CU : CUs   ' % ncu + ' ; '.join('%s: %d' % (','.join(map(str, k)), v) for k, v in sorted(gens.items(), key=lambda kv: -kv[1])[:6]))
