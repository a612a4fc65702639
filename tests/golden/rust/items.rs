//! Items of every kind the gate knows, with attributes, visibility and qualifiers in front of them.
#![allow(dead_code, unused_imports, unused_variables)]

use std::collections::{BTreeMap, HashMap};
use std::fmt::{self, Display, Formatter};
use std::sync::atomic::{AtomicU32, Ordering};

/// A field element below 2^31 - 1.
pub const MODULUS: u32 = (1 << 31) - 1;
pub(crate) static COUNTER: AtomicU32 = AtomicU32::new(0);
static mut SCRATCH: [u8; 4] = [0; 4];
type Map<K> = BTreeMap<K, Vec<u32>>;

/// A point on the circle, in projective form.
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq, Hash)]
#[repr(C)]
pub struct Point {
    /// first coordinate
    pub x: u32,
    /// second coordinate
    pub y: u32,
}

pub struct Wrapper<'a, T: ?Sized + 'a>(pub &'a T);

pub struct Unit;

#[derive(Debug)]
pub enum Shape<T = u32> {
    /// nothing at all
    Empty,
    Single(T),
    Pair(T, T),
    Named { first: T, second: Option<T> },
}

#[repr(C)]
pub union Bits {
    pub word: u32,
    pub bytes: [u8; 4],
}

pub trait Field: Copy + Sized + Display {
    const ZERO: Self;
    type Wide;

    fn add(self, other: Self) -> Self;
    fn double(self) -> Self {
        self.add(self)
    }
    fn name() -> &'static str
    where
        Self: 'static,
    {
        "field"
    }
}

impl Display for Point {
    fn fmt(&self, f: &mut Formatter<'_>) -> fmt::Result {
        write!(f, "({}, {})", self.x, self.y)
    }
}

impl<T: Clone> Shape<T> {
    pub const fn empty() -> Self {
        Shape::Empty
    }

    pub fn first(&self) -> Option<&T> {
        match self {
            Shape::Empty => None,
            Shape::Single(a) | Shape::Pair(a, _) => Some(a),
            Shape::Named { first, .. } => Some(first),
        }
    }
}

impl<'a, T: ?Sized> Wrapper<'a, T> {
    pub fn get(&self) -> &'a T {
        self.0
    }
}

pub mod nested {
    use super::Point;

    pub(super) fn origin() -> Point {
        Point { x: 0, y: 0 }
    }

    pub mod deeper {
        pub unsafe fn raw(p: *const u32) -> u32 {
            unsafe { *p }
        }
    }
}

#[allow(non_camel_case_types)]
#[repr(C)]
pub struct cm_pair {
    pub lo: u32,
    pub hi: u64,
    pub data: *const u32,
    pub rows: [u64; 4],
}

unsafe extern "C" {
    pub fn abs(x: i32) -> i32;
    pub fn strlen(s: *const core::ffi::c_char) -> usize;
}

pub extern "C" fn exported(x: u32) -> u32 {
    x.wrapping_mul(3)
}

pub async fn later(x: u32) -> u32 {
    x + 1
}

unsafe impl Send for Bits {}

impl Default for Bits {
    fn default() -> Self {
        Bits { word: 0 }
    }
}

macro_rules! square {
    ($x:expr) => {
        $x * $x
    };
    ($x:expr, $($rest:expr),+ $(,)?) => {
        square!($x) + square!($($rest),+)
    };
}

thread_local! {
    static DEPTH: std::cell::Cell<u32> = const { std::cell::Cell::new(0) };
}

pub fn sum_of_squares() -> u32 {
    square!(1u32, 2, 3,)
}

#[cfg(test)]
mod tests {
    use super::*;

    #[test]
    fn squares() {
        assert_eq!(sum_of_squares(), 14);
    }
}
