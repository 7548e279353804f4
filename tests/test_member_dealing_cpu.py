"""CPU: the chunk table and the queue size of the fused member kernel's dealt launches (greb_member.hip, greb_member_queue.h, greb_kernels.h:
chunk_table), as the library exports them -- the kernel walks the very table the host builds."""
import pytest

from greb_climate_model_amd import abi, engine

SCHEDULES = [abi.CHUNKS_HALVING, abi.CHUNKS_EQUAL, abi.CHUNKS_QUARTERS]


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_the_chunk_table_covers_the_steps_of_a_year_exactly_once_and_in_order(schedule):
    end = engine.member_chunk_table(schedule, abi.NSTEP_YR)
    assert 1 <= len(end) <= abi.MAX_CHUNKS
    steps, begin = [], 0
    for e in end:
        assert e > begin  # no empty chunk
        steps += list(range(begin + 1, e + 1))  # 1-based steps of the year
        begin = e
    assert steps == list(range(1, abi.NSTEP_YR + 1))


def test_the_schedules_are_the_documented_ones():
    end = engine.member_chunk_table(abi.CHUNKS_HALVING)
    assert [b - a for a, b in zip([0] + end, end)] == [365, 183, 91, 46, 23, 12, 10]
    end = engine.member_chunk_table(abi.CHUNKS_EQUAL)
    assert [b - a for a, b in zip([0] + end, end)] == [73] * 10
    end = engine.member_chunk_table(abi.CHUNKS_QUARTERS)
    assert [b - a for a, b in zip([0] + end, end)] == [183, 182, 183, 91, 46, 23, 12, 10]


@pytest.mark.parametrize("nsteps", [1, 2, 7, 100, 729, 731, 1460])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_other_step_counts_are_covered_without_empty_chunks(schedule, nsteps):
    end = engine.member_chunk_table(schedule, nsteps)
    assert end[-1] == nsteps and all(b > a for a, b in zip([0] + end, end)) and len(end) <= abi.MAX_CHUNKS


@pytest.mark.parametrize("members", [1, 3, 300, 384, 512, 4096])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_the_queue_capacity_is_members_times_chunks(schedule, members):
    assert engine.member_queue_capacity(members, schedule) == members * len(engine.member_chunk_table(schedule))


def test_bad_arguments_are_errors():
    with pytest.raises(engine.GrebError):
        engine.member_chunk_table(3)
    with pytest.raises(engine.GrebError):
        engine.member_chunk_table(abi.CHUNKS_HALVING, 0)
    with pytest.raises(engine.GrebError):
        engine.member_queue_capacity(0)
    assert "greb_engine_set_dealing" in engine.EXPORTS
