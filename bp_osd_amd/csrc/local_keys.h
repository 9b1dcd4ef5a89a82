// local_keys.h -- the key of a 64-position group of the local-edge BP kernel, shared by the kernel (bp_local_kernel.hip.h:
// which iteration-loop body a wave runs) and the host (local_layout.h: which groups share a wave).  Pure constexpr C++.
#pragma once

namespace bposd_local_keys {

// key = 4 * dl(slot 0) + dl(slot 1) of a group whose two slots are uniform with dl(slot 0) <= dl(slot 1) (the order
// class_sorted() gives every check); every other group -- a slot whose lanes differ (grp_dl == 3), or an order the host
// does not produce -- runs the per-lane selects on both slots: key 15.  Seven keys, one loop body each.
constexpr int kMixedKey = 15;
constexpr int kNumKeys = 7;
constexpr int kKeys[kNumKeys] = {0, 1, 2, 5, 6, 10, 15};  // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) mixed

constexpr int group_key(int dl0, int dl1) { return (dl0 >= 0 && dl0 <= dl1 && dl1 < 3) ? 4 * dl0 + dl1 : kMixedKey; }
constexpr int key_dl(int key, int slot) { return key == kMixedKey ? 3 : (slot == 0 ? key / 4 : key % 4); }

// Pair keys.  A wave of the two-checks-per-thread kernels whose first group has a uniform key k and whose second group is
// mixed (the host puts the mixed group second: local_layout::pair_groups) has the pair key 32 + k (decimal in the
// kernel's listing marker, which prints small constants only that way).  It is a
// property of the wave, not of a group (a group's key stays one of the seven above), and a kernel instance has a loop body
// for at most one of them (template parameter PAIRKEY = k of bp_local_kernel): the host picks the instance from the layout.
constexpr int kNumPairKeys = 6;
constexpr int kPairKeys[kNumPairKeys] = {32, 33, 34, 37, 38, 42};  // partner (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)

constexpr int pair_key(int k) { return (k >= 0 && k < kMixedKey) ? 32 + k : -1; }
constexpr bool is_pair_key(int key) { return key >= 32; }
// key of group j (0 / 1) of a wave that runs the loop body `key` (one of the seven, or a pair key)
constexpr int body_group_key(int key, int j) { return is_pair_key(key) ? (j == 0 ? key - 32 : kMixedKey) : key; }

}  // namespace bposd_local_keys
