"""numpy restatements of the reference's merge (IndexCreator::mergeTargetFiles<DB_CREATION> and
filterKmers<DB_CREATION>, IndexCreator.h:322-629) that the merge tests take their expected values from
(never from the code under test). tests/test_ref_merge.py holds them byte for byte to the reference's
own output (tests/golden/ref_merge.npz)."""
import numpy as np

from tests.dbref import diff_words


def merge_rule_split(values, n_before, split_num):
    """IndexCreator.h:432-447 restated: the split entries a merge writes, sizeOfSplit =
    numOfKmerBeforeMerge / (splitNum - 1)."""
    size = n_before // (split_num - 1)
    offset_list = [os_ * size for os_ in range(split_num)] + [None]
    split = np.zeros(3 * split_num, np.uint64)
    words = diff_words(values)
    aa = np.asarray(values, np.uint64) >> np.uint64(24)
    offset_idx, split_idx, check, aa_tmp = 1, 1, 0, None
    diff_cnt = 0
    for i in range(len(values)):
        info_cnt = i + 1
        diff_cnt += int(words[i])
        if check == 1 and int(aa[i]) != aa_tmp:
            split[3 * split_idx:3 * split_idx + 3] = (values[i], diff_cnt, info_cnt)
            split_idx += 1
            check = 0
        if info_cnt == offset_list[offset_idx]:
            aa_tmp = int(aa[i])
            check = 1
            offset_idx += 1
    return split


def expected_merge(tree, parts):
    """numpy concat, lexsort by (value, species, taxID), group-LCA over (value, species)."""
    v = np.concatenate([np.asarray(p[0], np.uint64) for p in parts])
    t = np.concatenate([np.asarray(p[1], np.int64) for p in parts])
    sp = tree.sp[t]
    order = np.lexsort((t, sp, v))
    v, t, sp = v[order], t[order], sp[order]
    if len(v) == 0:
        return v, t.astype(np.uint32)
    head = np.ones(len(v), bool)
    head[1:] = (v[1:] != v[:-1]) | (sp[1:] != sp[:-1])
    starts = np.flatnonzero(head)
    ends = np.concatenate([starts[1:], [len(v)]])
    info = t[starts].copy()
    for g in np.flatnonzero(ends - starts > 1):
        red = int(t[starts[g]])
        for x in t[starts[g] + 1:ends[g]].tolist():
            red = tree.lca(red, int(x))
        info[g] = red
    return v[starts], info.astype(np.uint32)
