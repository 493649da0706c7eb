"""The last-workgroup hand-off that closes every O(n) kernel of the single-problem solvers (optiml_amd/csrc/bq_reduce.h:
bq_part_put, bq_last_block, bq_part_get), tested directly through bq_ctx_probe_last_block: 200 launches back to back on the stream,
every workgroup stores one partial that depends on (workgroup, round), the workgroup that arrives last compares EVERY partial with
its expected word — its L1 warm with the previous round's words, with and without a workgroup-dependent amount of work before
the store.  One stale word in any round is a failure, and so is a ticket the last workgroup did not set back.  Sizes: one workgroup,
two, the edges of the 256-strided final reduction, and many more workgroups than the device holds at once."""
import pytest

pytestmark = pytest.mark.gpu

ROUNDS = 200


@pytest.fixture(scope='module')
def ctx():
    from optiml_amd import device
    return device.Context()


@pytest.mark.parametrize('uneven', [False, True], ids=['even', 'uneven'])
@pytest.mark.parametrize('blocks', [1, 2, 255, 256, 257, 1024, 4096])
def test_last_block_sees_every_partial_and_resets_the_ticket(ctx, blocks, uneven):
    bad, ticket = ctx.probe_last_block(blocks, rounds=ROUNDS, uneven=uneven)
    print(f'blocks={blocks} uneven={uneven}: {bad} stale words of {blocks * ROUNDS}, ticket {ticket}')
    assert bad == 0
    assert ticket == 0
