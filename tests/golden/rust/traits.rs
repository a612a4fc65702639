//! Traits with generic and associated items, operator impls, iterators, `impl Trait` and `dyn Trait`.
use std::iter::FromIterator;
use std::marker::PhantomData;
use std::ops::{Add, Index, IndexMut, Mul};

#[derive(Clone, Copy, Debug, PartialEq, Eq, PartialOrd, Ord)]
pub struct M31(pub u32);

impl M31 {
    pub const P: u32 = (1 << 31) - 1;

    #[inline]
    pub fn reduce(x: u64) -> Self {
        let lo = (x & Self::P as u64) + (x >> 31);
        let lo = (lo & Self::P as u64) + (lo >> 31);
        M31(if lo == Self::P as u64 { 0 } else { lo as u32 })
    }
}

impl Add for M31 {
    type Output = M31;
    fn add(self, rhs: M31) -> M31 {
        M31::reduce(self.0 as u64 + rhs.0 as u64)
    }
}

impl Mul for M31 {
    type Output = Self;
    fn mul(self, rhs: Self) -> Self::Output {
        M31::reduce(self.0 as u64 * rhs.0 as u64)
    }
}

pub trait Column: Index<usize, Output = M31> + IndexMut<usize> {
    fn len(&self) -> usize;
    fn is_empty(&self) -> bool {
        self.len() == 0
    }
}

#[derive(Default)]
pub struct Owned {
    data: Vec<M31>,
}

impl Index<usize> for Owned {
    type Output = M31;
    fn index(&self, i: usize) -> &M31 {
        &self.data[i]
    }
}

impl IndexMut<usize> for Owned {
    fn index_mut(&mut self, i: usize) -> &mut M31 {
        &mut self.data[i]
    }
}

impl Column for Owned {
    fn len(&self) -> usize {
        self.data.len()
    }
}

impl FromIterator<M31> for Owned {
    fn from_iter<I: IntoIterator<Item = M31>>(iter: I) -> Self {
        Owned { data: iter.into_iter().collect() }
    }
}

pub struct Evens<'a> {
    col: &'a Owned,
    at: usize,
}

impl<'a> Iterator for Evens<'a> {
    type Item = &'a M31;
    fn next(&mut self) -> Option<Self::Item> {
        let r = self.col.data.get(self.at);
        self.at += 2;
        r
    }
}

pub fn evens(col: &Owned) -> impl Iterator<Item = &M31> + '_ {
    Evens { col, at: 0 }
}

pub fn total(cols: &[&dyn Column]) -> M31 {
    cols.iter().fold(M31(0), |acc, c| (0..c.len()).fold(acc, |a, i| a + c[i]))
}

pub struct Typed<T> {
    raw: u32,
    _marker: PhantomData<fn() -> T>,
}

impl<T> Typed<T> {
    pub const fn new(raw: u32) -> Self {
        Typed { raw, _marker: PhantomData }
    }
}

pub trait Visitor {
    type Out;
    fn visit<V: AsRef<[u32]>>(&mut self, v: V) -> Self::Out;
}

impl<T> Visitor for Typed<T>
where
    T: Default,
{
    type Out = (u32, T);
    fn visit<V: AsRef<[u32]>>(&mut self, v: V) -> (u32, T) {
        self.raw += v.as_ref().iter().sum::<u32>();
        (self.raw, T::default())
    }
}

pub fn dispatch(v: &mut dyn FnMut(u32) -> u32, n: u32) -> u32 {
    (0..n).map(|i| v(i)).sum()
}
