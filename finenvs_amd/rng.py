"""Host mirror of the device redraw generator (Philox4x32-10, csrc/fe_env.hip:philox_u32).

Used to pick the eval env's first day in redraw="device" mode so that the
whole day sequence is a pure function of (seed, draw counter), and to mirror the
keyed permutation PPO's mini-batches are drawn from (``ppo_permute``)."""

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox_u32(seed: int, counter: int) -> int:
    c = [counter & _MASK, (counter >> 32) & _MASK, 0x46454E56, 0]
    k = [seed & _MASK, (seed >> 32) & _MASK]
    for _ in range(10):
        p0 = _M0 * c[0]
        p1 = _M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & _MASK, p1 & _MASK, ((p0 >> 32) ^ c[3] ^ k[1]) & _MASK, p0 & _MASK]
        k = [(k[0] + _W0) & _MASK, (k[1] + _W1) & _MASK]
    return c[0]


def redraw_day(seed: int, counter: int, num_days: int) -> int:
    return (philox_u32(seed, counter) * num_days) >> 32


from ._lib import PPO_PERM_SALT  # FE_PPO_PERM_SALT of include/finenvs_amd_ppo.h
_MASK64 = 0xFFFFFFFFFFFFFFFF


def ppo_permute(seed: int, epoch: int, n: int, i: int) -> int:
    """Host mirror of ``fe_ppo_minibatch``'s keyed permutation (include/finenvs_amd_ppo.h): where position ``i`` of epoch
    ``epoch``'s shuffle of ``[0, n)`` goes.  A four-round balanced Feistel network over ``2 * hb`` bits with
    ``philox_u32`` as its round function, walked until the value falls below ``n``; a bijection of ``[0, n)`` for every
    ``(seed, epoch)``.  ``1 <= n < 2**32``, ``0 <= i < n``."""
    n, i = int(n), int(i)
    if not 1 <= n < 1 << 32 or not 0 <= i < n:
        raise ValueError(f"ppo_permute needs 1 <= n < 2**32 and 0 <= i < n (got n = {n}, i = {i})")
    k = max(1, (n - 1).bit_length())
    hb = (k + 1) // 2
    mask = (1 << hb) - 1
    key = (int(seed) ^ PPO_PERM_SALT) & _MASK64
    epoch4 = (int(epoch) * 4) & _MASK64
    x = i
    for _ in range(1 << (2 * hb)):  # the walk is bounded by the domain's size, as on the device
        l, r = x >> hb, x & mask
        for rnd in range(4):
            counter = ((((epoch4 + rnd) & _MASK64) << 16) & _MASK64) | r
            l, r = r, l ^ (philox_u32(key, counter) & mask)
        x = (l << hb) | r
        if x < n:
            return x
    return -1
