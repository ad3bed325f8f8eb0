"""CPU: merlin.task_mix (mixture strings -> per-env difficulty assignments) and the scenario creator's mixture
checks."""
import itertools

import pytest

ORDER = ["easy", "medium", "mediumhard", "hard", "hardest"]


def runs_of(names):
    return [(d, len(list(g))) for d, g in itertools.groupby(names)]


def test_parse_mix_round_trips():
    from merlin.task_mix import format_mix, parse_mix

    w = parse_mix("easy:1,mediumhard:2,hard:1")
    assert w == {"easy": 1.0, "mediumhard": 2.0, "hard": 1.0} and list(w) == ["easy", "mediumhard", "hard"]
    assert parse_mix(format_mix(w)) == w
    assert parse_mix(" hard : 0.25 , easy:3 ") == {"hard": 0.25, "easy": 3.0}
    assert parse_mix("medium") == {"medium": 1.0}
    assert parse_mix({"easy": 2, "hardest": 1}) == {"easy": 2.0, "hardest": 1.0}
    w = {"easy": 1 / 3, "hard": 1e-3}
    assert parse_mix(format_mix(w)) == w


@pytest.mark.parametrize("spec", ["nope:1", "easy:1,Hard:2", "easy:0", "easy:-1", "easy:x", "easy:nan", "easy:inf",
                                  "easy:1,easy:2", "", ",", {"easy": 0.0}, {"trivial": 1}])
def test_parse_mix_rejects(spec):
    from merlin.task_mix import parse_mix

    with pytest.raises(ValueError):
        parse_mix(spec)


def test_assign_aligned_runs():
    from merlin.task_mix import assign

    names = assign(4096, {"easy": 1, "mediumhard": 2, "hard": 1})
    assert runs_of(names) == [("easy", 1024), ("mediumhard", 2048), ("hard", 1024)]
    assert names == assign(4096, "hard:1,mediumhard:2,easy:1")  # deterministic; the order is the generators', not the
    # string's
    names = assign(4096, {d: 1 for d in ORDER})
    runs = runs_of(names)
    assert [d for d, _ in runs] == ORDER and sum(r for _, r in runs) == 4096
    edge = 0
    for _, r in runs[:-1]:
        edge += r
        assert edge % 64 == 0
    assert sorted(r for _, r in runs) == [768, 832, 832, 832, 832]  # 64 units of 64 envs: 12 or 13 each


def test_assign_small_and_unaligned():
    from merlin.task_mix import assign

    assert runs_of(assign(10, {d: 1 for d in ORDER})) == [(d, 2) for d in ORDER]
    assert runs_of(assign(256, {"easy": 1, "hard": 1})) == [("easy", 128), ("hard", 128)]
    # 300 envs, 3 classes: 5 units of 64 (the last partial, with the last class)
    runs = runs_of(assign(300, {"easy": 1, "medium": 1, "hard": 1}))
    assert sum(r for _, r in runs) == 300 and all(r % 64 == 0 for _, r in runs[:-1])
    with pytest.raises(ValueError):
        assign(2, {"easy": 1, "medium": 1, "hard": 1})


def test_assign_length_and_minimum_share():
    """The length is num_envs and a class with a positive weight never gets 0 envs, however small its weight."""
    from merlin.task_mix import assign

    for n in (3, 5, 7, 63, 64, 65, 191, 192, 193, 320, 321, 1000, 4096, 4097):
        for weights in ({"easy": 1000, "hard": 1e-6, "hardest": 1}, {"medium": 1, "mediumhard": 1e9},
                        {d: i + 1 for i, d in enumerate(ORDER)}):
            if n < len(weights):
                continue
            for align in (64, 1, 16):
                names = assign(n, weights, align=align)
                assert len(names) == n, (n, weights, align)
                got = dict(runs_of(names))
                assert set(got) == set(weights) and min(got.values()) >= 1, (n, weights, align)
                assert [d for d, _ in runs_of(names)] == [d for d in ORDER if d in weights]
                assert names == assign(n, weights, align=align)


YAML = """
global:
  max_steps: 64
difficulties:
  easy:
    env_id: MERLIN-Easy-v0
    params: {render_mode: rgb_array, size: 16}
  medium:
    env_id: MERLIN-Medium-v0
    params: {render_mode: rgb_array, size: 16}
  hard:
    env_id: MERLIN-Hard-v0
    params: {render_mode: rgb_array, size: 16, max_steps: 99}
"""


def test_mix_env_kwargs(tmp_path):
    """The env kwargs of a mixture: per-env generators from assign, everything else shared; difficulties whose other
    kwargs differ (here max_steps) are refused.  No env is created: no GPU."""
    from merlin.scenario_creator import ScenarioCreator

    path = tmp_path / "scenario.yaml"
    path.write_text(YAML)
    sc = ScenarioCreator(str(path))
    assert sc._env_kwargs("easy") == {"difficulty": "easy", "size": 16, "max_steps": 64}
    kw = sc._mix_env_kwargs("easy:1,medium:3", 256)
    assert kw["size"] == 16 and kw["max_steps"] == 64
    assert runs_of(kw["difficulty"]) == [("easy", 64), ("medium", 192)]
    assert sc._mix_env_kwargs({"medium": 1, "easy": 1}, 6)["difficulty"] == ["easy"] * 3 + ["medium"] * 3
    with pytest.raises(ValueError, match="max_steps"):
        sc._mix_env_kwargs("easy:1,hard:1", 256)
    with pytest.raises(ValueError):
        sc.create_vec_env("easy:1,hard:1", 256)  # raises before any env is created
    with pytest.raises(ValueError):
        sc._mix_env_kwargs("easy:1,hardest:1", 256)  # not in this config
