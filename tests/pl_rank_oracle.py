"""The polisher's rule 2 in ranked form and rule 1's check (j), restated in plain Python around tests/pl_oracle.py: everything
behind the voters is pl_oracle's.  A rank row is (parent, sub, n_secondary, mapq), as tests/map_rank_oracle.py gives it."""
import pl_oracle


def bad_rank(chains, ranks, i):
    """rule 1 (j) for chain i"""
    parent, _, _, mapq = ranks[i]
    if not 0 <= parent < len(chains) or mapq > 60:
        return True
    return chains[parent][0] != chains[i][0] or ranks[parent][0] != parent


def check(draft, reads, chains, runs, ranks):
    """rule 1 with (j): the smallest bad chain, and of that chain (j) last"""
    assert len(ranks) == len(chains)
    first = next((i for i in range(len(chains)) if bad_rank(chains, ranks, i)), None)
    try:
        pl_oracle.check(draft, reads, chains, runs)
    except pl_oracle.PolishError as e:
        if first is None or e.chain <= first:
            raise
    if first is not None:
        raise pl_oracle.PolishError(first, "rank")


def voters(chains, ranks, min_identity, min_mapq):
    """rule 2, ranked: eligible, primary, and of sufficient mapping quality"""
    return [i for i, ch in enumerate(chains)
            if ch[10] * 100 >= min_identity * ch[11] and ranks[i][0] == i and ranks[i][3] >= min_mapq]


def run(draft, reads, chains, runs, ranks, min_mapq=0, **params):
    """pl_oracle.run with the ranked voters; ``voters`` of the result lists them"""
    check(draft, reads, chains, runs, ranks)
    plain = pl_oracle.voters
    pl_oracle.voters = lambda table, min_identity: voters(table, ranks, min_identity, min_mapq)
    try:
        return pl_oracle.run(draft, reads, chains, runs, **params)
    finally:
        pl_oracle.voters = plain
