"""The polisher's rule 2 in mates form and rule 1's check (k), restated in plain Python around tests/pl_oracle.py: everything
behind the voters is pl_oracle's.  A mate row is (mate, tlen, cls, n_best), as tests/map_mate_oracle.py gives it."""
import pl_oracle


def bad_mate(chains, mates, i):
    """rule 1 (k) for chain i"""
    mate, _, cls, n_best = mates[i]
    if cls > 1:
        return True
    if cls == 0:
        return False
    if not 0 <= mate < len(chains) or n_best < 1:
        return True
    return mates[mate][2] != 1 or mates[mate][0] != i or chains[mate][0] != chains[i][0] ^ 1


def check(draft, reads, chains, runs, mates):
    """rule 1 with (k): the smallest bad chain, and of that chain (k) last"""
    assert len(mates) == len(chains)
    first = next((i for i in range(len(chains)) if bad_mate(chains, mates, i)), None)
    try:
        pl_oracle.check(draft, reads, chains, runs)
    except pl_oracle.PolishError as e:
        if first is None or e.chain <= first:
            raise
    if first is not None:
        raise pl_oracle.PolishError(first, "mates")


def voters(chains, mates, min_identity):
    """rule 2, mates form: eligible, selected, and the pair placed best once"""
    return [i for i, ch in enumerate(chains) if ch[10] * 100 >= min_identity * ch[11] and mates[i][2] == 1 and mates[i][3] == 1]


def run(draft, reads, chains, runs, mates, **params):
    """pl_oracle.run with the mates voters; ``voters`` of the result lists them"""
    check(draft, reads, chains, runs, mates)
    plain = pl_oracle.voters
    pl_oracle.voters = lambda table, min_identity: voters(table, mates, min_identity)
    try:
        return pl_oracle.run(draft, reads, chains, runs, **params)
    finally:
        pl_oracle.voters = plain
